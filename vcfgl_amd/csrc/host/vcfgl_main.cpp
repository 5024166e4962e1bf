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
//     genotype gets GL 0 / GP 1 / PL 0 and every other genotype -inf / 0 / 255; written directly
//   * -printTruth 1: the decoded input records (incl. exploded ones) as <prefix>.truth.vcf
// CPU simulation path here.  Input: VCF text, gzip / bgzip'd VCF, BCF (raw or BGZF).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <errno.h>
#include <string.h>
#include <time.h>
#include <zlib.h>

#include <algorithm>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/vcfgl_hip.h"
#include "vcf_sink.h"

// Records are parsed, simulated and encoded on several threads, and any of them may hit a fatal input error: the first
// one reports and leaves through _exit() (no static destructors run under the feet of the threads still working, which is
// what exit() from two threads at once did), the others park.
#include <atomic>
#include <unistd.h>
static std::atomic<bool> g_dying{false};
[[noreturn]] static void die_v(const char* fmt, va_list ap) {
    if (g_dying.exchange(true)) for (;;) pause();
    fflush(stdout);
    fprintf(stderr, "\n\n*******\n[ERROR] "); vfprintf(stderr, fmt, ap); fprintf(stderr, "\n*******\n");
    fflush(NULL);
    _exit(1);                                  // shared.h:292-299 exit(1)
}
[[noreturn]] static void die(const char* fmt, ...) { va_list ap; va_start(ap, fmt); die_v(fmt, ap); }
[[noreturn]] void vsink::fail(const char* fmt, ...) { va_list ap; va_start(ap, fmt); die_v(fmt, ap); }

// ---------------------------------------------------------------------------------------
struct Args {
    int seed = -1, source = 0, error_qs = 0, gl_model = 2, precise_gl = 0, i16_mapq = 20, adjust_qs = 0;
    int explode = 0, rm_invar = 0, rm_empty = 0, do_unobserved = 1, do_gvcf = 0, print_pileup = 0, print_truth = 0;
    int print_bpe = 0, print_qs_err = 0, print_gl_err = 0, print_qscores = 0;     // per-read / per-site TSV lines on stdout
    int add_gl = 1, add_gp = 0, add_pl = 0, add_i16 = 0, add_qs = 0, add_fmt_dp = 1, add_info_dp = 0;
    int add_fmt_ad = 0, add_info_ad = 0, add_fmt_adf = 0, add_info_adf = 0, add_fmt_adr = 0, add_info_adr = 0;
    int rng_mode = VGL_RNG_TILE, beta_sampler = -1, tile_sites = 4096, device = 0, verbose = 0, threads = 1, enc_threads = 0;
    bool threads_given = false;
    int device_bgzf = 0;               // --device-bgzf 1: BGZF streams compressed on the first device of the run
    int device_text = 0;               // --device-text 1: the sample columns of VCF text records formatted on the device
    int device_bcf = 0;                // --device-bcf 1: the FORMAT part of BCF records (-O u / -O b) encoded on the device
    int device_gvcf = 0;               // --device-gvcf 1: -doGVCF 1 blocks built and their / the records' sample columns formatted on the device
    int device_pileup = 0;             // --device-pileup 1: the N-wide part of -printPileup 1's lines formatted on the device
    int device_stream = 0;             // --device-stream 1: a tile's records assembled and BGZF-compressed on the device that simulated it
    int gt_disc = 0;                   // --gt-discordance 1: calls tallied against the truth on the device, <prefix>.discordance.tsv
    int disc_gq = 0;                   // --discordance-gq 0|3|4|5|6: gtDiscordance's -doGQ layout of that file
    int records = 1;                   // --records 0: no record file; only the discordance table comes back
    int device_inflate = 0;            // --device-inflate 1: a BGZF input is inflated on the first device of the run
    int device_input = 0;              // --device-input 1: the sample columns of the input VCF text parsed on the first device of the run
    double depth = -1.0, error_rate = -1.0, beta_variance = -1.0, gl1_theta = 0.83, adjust_by = 0.499;
    bool have_depth = false, depth_inf = false;
    std::string in_fn, out_prefix = "output", output_mode = "b", depths_fn, qs_bins_fn, command;
    std::vector<double> depths;
    std::vector<int32_t> qs_bins;
    std::string gvcf_dps_str;
    std::vector<int> gvcf_dps;
    std::vector<int> devices;          // --devices 0,1,...: one context + host thread per GPU, tiles dealt round robin
};

static const char USAGE[] =
    "\nvcfgl_hip: genotype-likelihood simulation on an MI355X (vcfgl's flags; every flag takes one value)\n\n"
    "Usage: vcfgl_hip -i <in.vcf|vcf.gz|bcf> -e <error rate> -d <depth>|inf | -df <depths file> [options]\n\n"
    "  input / output   -i --input FILE    -o --output PREFIX [output]    -O --output-mode b|u|z|v [b]    --source 0|1 [0: binary alleles, 1: ACGT]\n"
    "                   -@ --threads INT [1]    -V --verbose INT [0]    -s --seed INT [time]\n"
    "  depth            -d --depth FLOAT|inf    -df --depths-file FILE (one mean depth per sample)\n"
    "  errors           -e --error-rate FLOAT    -eq --error-qs 0|1|2 [0]    -bv --beta-variance FLOAT    --qs-bins FILE (lo,hi,value per line)\n"
    "                   --adjust-qs 0..31 [0: bit 1 GL, 2 QS tag, 4 pileup, 8 -printQScores, 16 -printGlError]    --adjust-by FLOAT [0.499]\n"
    "  likelihoods      -GL --gl-model 1|2 [2]    --gl1-theta FLOAT [0.83]    --precise-gl 0|1 [0]    --i16-mapq INT [20]\n"
    "  sites            -explode 0|1 [0]    --rm-invar-sites 0..7 [0]    --rm-empty-sites 0|1 [0]    -doUnobserved 0..5 [1]\n"
    "                   -doGVCF 0|1 [0]    --gvcf-dps INT,INT,... (with -doGVCF 1)\n"
    "  tags             -addGL [1] -addGP [0] -addPL [0] -addI16 [0] -addQS [0] -addFormatDP [1] -addInfoDP [0]\n"
    "                   -addFormatAD -addInfoAD -addFormatADF -addInfoADF -addFormatADR -addInfoADR [0]\n"
    "  extra files      -printPileup 0|1 (<prefix>.pileup.gz)    -printTruth 0|1 (<prefix>.truth.*)\n"
    "  lines on stdout  -printBasePickError -printQsError -printGlError -printQScores 0|1\n"
    "  this program     --rng-mode 0|1 [0: counter-addressed windows of the rand48 sequence (fast, shards over GPUs);\n"
    "                                   1: the reference program's own draw order (reproduces its output)]\n"
    "                   --beta-sampler 0|1 [0: the rand48 sampler, 1: std::mt19937 (default with --rng-mode 1)]\n"
    "                   --tile-sites INT [4096]    --device INT [0]    --devices INT,INT,... (several GPUs of the node: sites shard by\n"
    "                   absolute index, the output does not depend on the device count; --rng-mode 0 only)    --encode-threads INT\n"
    "                   --device-bgzf 0|1 [0: BGZF members compressed by zlib on the host; 1: on the first GPU of --device / --devices,\n"
    "                   for every BGZF stream the run writes (-O b / -O z output, truth file, -printPileup's .pileup.gz; with -O u / -O v\n"
    "                   the output and truth files are not BGZF and the flag changes nothing there).  Same decompressed bytes either way;\n"
    "                   a run without a GPU fails instead of falling back, --depth inf included]\n"
    "                   --device-text 0|1 [0: the sample columns of -O v / -O z records formatted on the host; 1: on the device that\n"
    "                   simulated the tile, and the text crosses the link instead of the FORMAT arrays.  Same bytes either way; needs -O v\n"
    "                   or -O z, refused with -doGVCF 1 and --depth inf; a run without a GPU fails instead of falling back]\n"
    "                   --device-gvcf 0|1 [0: -doGVCF 1 blocks built on the host, site by site; 1: on the device that simulated the tile,\n"
    "                   with the sample columns of records and blocks formatted there (blocks that cross a tile are merged on the host).\n"
    "                   Same bytes either way; needs -doGVCF 1 and -O v or -O z (-O u / -O b with --device-bcf 1), refused with --depth inf;\n"
    "                   a run without a GPU fails]\n"
    "                   --device-bcf 0|1 [0: the FORMAT arrays of -O u / -O b records typed and narrowed on the host; 1: encoded as BCF typed\n"
    "                   vectors on the device that simulated the tile, and the encoded bytes cross the link instead of the FORMAT arrays.\n"
    "                   Same bytes either way; needs -O u or -O b, refused with --depth inf and with -doGVCF 1 unless --device-gvcf 1 is\n"
    "                   given too (which it then allows with -O u / -O b); a run without a GPU fails instead of falling back]\n"
    "                   --device-pileup 0|1 [0: -printPileup 1's lines formatted on the host from the read dump; 1: their sample columns\n"
    "                   formatted on the device that simulated the tile, and the text crosses the link instead of the read dump.  Same\n"
    "                   bytes either way; needs -printPileup 1, refused with --depth inf; a run without a GPU fails instead of falling back]\n"
    "                   --device-stream 0|1 [0: the records of -O b / -O z are put together on the host and compressed in batches; 1: a tile's\n"
    "                   records are assembled and BGZF-compressed on the device that simulated the tile: only the host-built heads (the\n"
    "                   fixed columns) go up and only compressed members come down.  The file decompresses to the same bytes; its\n"
    "                   members restart at every tile (more and shorter members), the EOF member ends it once.  Needs -O b with\n"
    "                   --device-bcf 1 or -O z with --device-text 1, refused with -doGVCF 1 and --depth inf; a run without a GPU fails]\n"
    "                   --gt-discordance 0|1 [0; 1: every simulated tile is genotyped on the device that simulated it (maximum-likelihood call\n"
    "                   from PL over the A/C/G/T genotypes, GQ = the second smallest PL capped at 127) and compared with its true genotypes;\n"
    "                   the counts are written to <prefix>.discordance.tsv, what misc/gtDiscordance prints for the records and -printTruth's\n"
    "                   file.  Works with every output mode, --device-* path, --devices and --rng-mode; refused with --depth inf]\n"
    "                   --discordance-gq 0|3|4|5|6 [0: gtDiscordance's -doGQ layout of that file: 0 one line per sample, 3 / 4 counts by GQ\n"
    "                   over all samples, 5 / 6 by sample and GQ (7 and 8 equal 6 here: every call has a GQ)]\n"
    "                   --records 0|1 [1; 0: no record file is opened and no FORMAT array, text or encoded record crosses the link: only the\n"
    "                   discordance table comes back.  Needs --gt-discordance 1; refused with -printPileup 1, -printTruth 1, -doGVCF 1 and\n"
    "                   the per-read listings]\n"
    "                   --device-input 0|1 [0: the genotype columns of the input VCF are parsed on the host; 1: on the first GPU of --device /\n"
    "                   --devices: the host reads the file, finds the lines and parses their first nine columns, the text goes up in batches of\n"
    "                   --tile-sites lines and one packed byte per sample comes back.  A line outside the plain grammar (GT alleles of '.' or\n"
    "                   one or two digits, at most two of them) is parsed by the host as with 0.  Same output either way; VCF text input only\n"
    "                   (BCF input is refused), refused with --depth inf; a run without a GPU fails instead of falling back]\n"
    "                   --device-inflate 0|1 [0: the input is read and inflated by zlib on one host thread; 1: a BGZF input (bgzip'd VCF text, compressed\n"
    "                   BCF) is read as it lies in the file and its members are inflated on the first GPU of --device / --devices, 512 members\n"
    "                   a batch.  A file that is not BGZF (plain text, gzip) and a file with a member the device does not take to its exact end\n"
    "                   are read by zlib as with 0: same bytes either way.  Refused with --depth inf; a run without a GPU fails instead of\n"
    "                   falling back]\n"
    "                   -v --version    -vv    -h --help\n\n";

static Args parse_args(int argc, char** argv) {
    Args a;
    a.command = "Command: vcfgl_hip";
    for (int i = 1; i < argc; i++) { a.command += " "; a.command += argv[i]; }
    auto I = [&](const char* v) { return atoi(v); };
    auto D = [&](const char* v) { return atof(v); };
    // io.cpp:538-752 compares the long simulation flags with strcasecmp (--error-qs, -addGL, -printPileup, -GL, -bv, -eq ...) and the
    // short / common ones (-s, -i, -o, -O, -d, -e, -V, -@ and their long forms) with strcmp: the former are matched in any case here too
    static const char* const nocase[] = {"--adjust-by", "--adjust-qs", "--beta-variance", "--error-qs", "--gl-model", "--gl1-theta", "--gvcf-dps",
        "--i16-mapq", "--precise-gl", "--qs-bins", "--rm-empty-sites", "--rm-invar-sites", "-GL", "-addFormatAD", "-addFormatADF", "-addFormatADR",
        "-addFormatDP", "-addFormatGL", "-addFormatGP", "-addFormatI16", "-addFormatPL", "-addFormatQS", "-addGL", "-addGP", "-addI16", "-addInfoAD",
        "-addInfoADF", "-addInfoADR", "-addInfoDP", "-addPL", "-addQS", "-bv", "-doGVCF", "-doUnobserved", "-eq", "-explode", "-printBasePickError",
        "-printGlError", "-printPileup", "-printQScores", "-printQsError", "-printTruth"};
    for (int i = 1; i < argc; i += 2) {
        std::string f = argv[i];
        for (const char* c : nocase) if (strcasecmp(c, f.c_str()) == 0) { f = c; break; }
        if (f == "-h" || f == "--help") { fputs(USAGE, stderr); exit(0); }
        if (f == "--version" || f == "-v") { fprintf(stderr, "vcfgl_hip [libvcfgl_hip ABI %d] [gfx950] [flag surface of vcfgl v1.3.0]\n\n", vgl_abi_version()); exit(0); }
        if (f == "-vv") { fprintf(stderr, "libvcfgl_hip ABI %d\n", vgl_abi_version()); exit(0); }
        if (i + 1 >= argc) die("Argument %s requires a value", argv[i]);
        const char* v = argv[i + 1];
        if (f == "--seed" || f == "-s") a.seed = I(v);
        else if (f == "--input" || f == "-i") a.in_fn = v;
        else if (f == "--source") a.source = I(v);
        else if (f == "--output" || f == "-o") a.out_prefix = v;
        else if (f == "--output-mode" || f == "-O") a.output_mode = v;
        else if (f == "--depth" || f == "-d") {
            if (!strcmp(v, "inf")) { a.depth_inf = true; a.depth = 0.0; }
            else a.depth = D(v);
            a.have_depth = true;
        } else if (f == "--depths-file" || f == "-df") a.depths_fn = v;
        else if (f == "--error-rate" || f == "-e") a.error_rate = D(v);
        else if (f == "--error-qs" || f == "-eq") a.error_qs = I(v);
        else if (f == "--beta-variance" || f == "-bv") a.beta_variance = D(v);
        else if (f == "--gl-model" || f == "-GL") a.gl_model = I(v);
        else if (f == "--gl1-theta") a.gl1_theta = D(v);
        else if (f == "--qs-bins") a.qs_bins_fn = v;
        else if (f == "--precise-gl") a.precise_gl = I(v);
        else if (f == "--i16-mapq") a.i16_mapq = I(v);
        else if (f == "--gvcf-dps") a.gvcf_dps_str = v;
        else if (f == "--adjust-qs") a.adjust_qs = I(v);
        else if (f == "--adjust-by") a.adjust_by = D(v);
        else if (f == "-explode") a.explode = I(v);
        else if (f == "--rm-invar-sites") a.rm_invar = I(v);
        else if (f == "--rm-empty-sites") a.rm_empty = I(v);
        else if (f == "-doUnobserved") a.do_unobserved = I(v);
        else if (f == "-doGVCF") a.do_gvcf = I(v);
        else if (f == "-printPileup") a.print_pileup = I(v);
        else if (f == "-printTruth") a.print_truth = I(v);
        else if (f == "-printBasePickError") a.print_bpe = I(v);
        else if (f == "-printQsError") a.print_qs_err = I(v);
        else if (f == "-printGlError") a.print_gl_err = I(v);
        else if (f == "-printQScores") a.print_qscores = I(v);
        else if (f == "-addGL" || f == "-addFormatGL") a.add_gl = I(v);
        else if (f == "-addGP" || f == "-addFormatGP") a.add_gp = I(v);
        else if (f == "-addPL" || f == "-addFormatPL") a.add_pl = I(v);
        else if (f == "-addI16" || f == "-addFormatI16") a.add_i16 = I(v);
        else if (f == "-addQS" || f == "-addFormatQS") a.add_qs = I(v);
        else if (f == "-addFormatDP") a.add_fmt_dp = I(v);
        else if (f == "-addInfoDP") a.add_info_dp = I(v);
        else if (f == "-addFormatAD") a.add_fmt_ad = I(v);
        else if (f == "-addInfoAD") a.add_info_ad = I(v);
        else if (f == "-addFormatADF") a.add_fmt_adf = I(v);
        else if (f == "-addInfoADF") a.add_info_adf = I(v);
        else if (f == "-addFormatADR") a.add_fmt_adr = I(v);
        else if (f == "-addInfoADR") a.add_info_adr = I(v);
        else if (f == "--verbose" || f == "-V") a.verbose = I(v);
        else if (f == "--threads" || f == "-@") { a.threads = I(v); a.threads_given = true; }
        else if (f == "--encode-threads") a.enc_threads = I(v);      // extension: record-encoding threads (any output mode)
        // extensions of this implementation
        else if (f == "--rng-mode") a.rng_mode = I(v);
        else if (f == "--beta-sampler") a.beta_sampler = I(v);
        else if (f == "--tile-sites") a.tile_sites = I(v);
        else if (f == "--device") a.device = I(v);
        else if (f == "--device-bgzf") a.device_bgzf = I(v);
        else if (f == "--device-text") a.device_text = I(v);
        else if (f == "--device-gvcf") a.device_gvcf = I(v);
        else if (f == "--device-bcf") a.device_bcf = I(v);
        else if (f == "--device-pileup") a.device_pileup = I(v);
        else if (f == "--device-stream") a.device_stream = I(v);
        else if (f == "--gt-discordance") a.gt_disc = I(v);
        else if (f == "--discordance-gq") a.disc_gq = I(v);
        else if (f == "--records") a.records = I(v);
        else if (f == "--device-input") a.device_input = I(v);
        else if (f == "--device-inflate") a.device_inflate = I(v);
        else if (f == "--devices") { a.devices.clear(); for (const char* q = v; *q;) { char* e; const long d = strtol(q, &e, 10); if (e == q || d < 0) die("Could not parse --devices %s", v); a.devices.push_back((int)d); q = (*e == ',') ? e + 1 : e; if (*e && *e != ',') die("Could not parse --devices %s", v); } }
        else die("Unknown argument: %s", argv[i]);
    }
    // ---- validation (io.cpp:757-1000, the rules that concern the hot path)
    auto range = [&](double v, double lo, double hi, const char* s) { if (v < lo || v > hi) die("[Bad argument value: '%s %g'] Allowed range is [%g,%g]", s, v, lo, hi); };
    if (a.in_fn.empty()) die("Input file is not specified. Please use -i/--input option to specify the input file.");
    if (!a.have_depth && a.depths_fn.empty()) die("Average per-site read depth value is required. Please set it using --depth or --depths-file and re-run.");
    if (a.depths_fn.empty()) range(a.depth, 0.0, 500.0, "--depth");
    range(a.device_stream, 0, 1, "--device-stream");
    // the discordance tally and a run without records (checked before any GPU work: nothing is written)
    range(a.gt_disc, 0, 1, "--gt-discordance"); range(a.records, 0, 1, "--records");
    if (a.disc_gq != 0 && (a.disc_gq < 3 || a.disc_gq > 6)) die("[Bad argument value: '--discordance-gq %d'] Allowed values are 0, 3, 4, 5, 6", a.disc_gq);
    if (a.disc_gq != 0 && !a.gt_disc) die("--discordance-gq %d selects the layout of --gt-discordance 1's file: add --gt-discordance 1.", a.disc_gq);
    if (a.gt_disc && a.depth_inf) die("--gt-discordance 1 is not supported with --depth inf (no tile is simulated: every call would be the truth).");
    if (!a.records) {
        if (!a.gt_disc) die("--records 0 writes no record file: it needs --gt-discordance 1, whose table is then the run's only output.");
        if (a.print_pileup) die("--records 0 is not supported with -printPileup 1 (the pileup is a listing of every read).");
        if (a.print_truth) die("--records 0 is not supported with -printTruth 1 (the truth file is a record file).");
        if (a.do_gvcf) die("--records 0 is not supported with -doGVCF 1 (gVCF blocks are records).");
        if (a.print_bpe || a.print_qs_err || a.print_gl_err || a.print_qscores)
            die("--records 0 is not supported with -printBasePickError / -printQsError / -printGlError / -printQScores 1 (per-read listings).");
        a.device_text = a.device_bcf = a.device_gvcf = a.device_stream = a.device_pileup = 0;      // nothing to format, encode or assemble
    }
    range(a.device_input, 0, 1, "--device-input");
    if (a.device_input == 1 && a.depth_inf) die("--device-input 1 is not supported with --depth inf (no device is used).");
    range(a.device_inflate, 0, 1, "--device-inflate");
    if (a.device_inflate == 1 && a.depth_inf) die("--device-inflate 1 is not supported with --depth inf (no device is used).");
    if (a.device_stream == 1 && a.depth_inf) die("--device-stream 1 is not supported with --depth inf (no tile is simulated).");
    if (a.device_gvcf == 1 && a.depth_inf) die("--device-gvcf 1 is not supported with --depth inf (no tile is simulated).");
    if (a.device_bcf == 1 && a.depth_inf) die("--device-bcf 1 is not supported with --depth inf (no tile is simulated).");
    if (a.depth_inf) {                                                          // io.cpp:781-850, 1011-1018
        if (a.rm_invar & 4) die("[--rm-invar-sites %d] Cannot skip invariable sites when --depth inf is set.", a.rm_invar);
        if (a.do_gvcf) die("[-doGVCF 1] Cannot output gVCF when --depth inf is set.");
        if (a.add_qs) die("(-addQS 1) QS tag cannot be added when --depth inf is set.");
        if (a.add_i16) die("(-addI16 1) I16 tag cannot be added when --depth inf is set.");
    }
    if (a.error_rate < 0) die("Error rate is not specified. Please use --error-rate option to specify the error rate. Allowed range: [0.0, 1.0]");
    if (a.error_rate >= 1.0) die("[Bad argument value: '--error-rate %f'] Allowed range is [0.0,1.0]", a.error_rate);
    range(a.source, 0, 1, "--source"); range(a.error_qs, 0, 2, "--error-qs"); range(a.gl_model, 1, 2, "--gl-model");
    range(a.gl1_theta, 0, 1, "--gl1-theta"); range(a.precise_gl, 0, 1, "--precise-gl"); range(a.i16_mapq, 0, 60, "--i16-mapq");
    range(a.adjust_qs, 0, 31, "--adjust-qs"); range(a.do_unobserved, 0, 5, "-doUnobserved"); range(a.rm_invar, 0, 7, "--rm-invar-sites");
    if (a.adjust_qs && a.adjust_by == 0.0) die("--adjust-qs %d requires a non-zero value for --adjust-by. Please set --adjust-by and rerun.", a.adjust_qs);
    if ((a.adjust_qs & 1) && a.precise_gl) die("--adjust-qs 1 requires --precise-gl 0. Please set --precise-gl 0 and rerun.");
    if ((a.adjust_qs & 2) && !a.add_qs) die("--adjust-qs 2 requires -addQS 1. Please set -addQS 1 and rerun.");
    if ((a.adjust_qs & 4) && !a.print_pileup) die("--adjust-qs 4 requires --printPileup 1. Please set --printPileup 1 and rerun.");   // io.cpp:891-898
    if ((a.adjust_qs & 8) && !a.print_qscores) die("--adjust-qs 8 requires --printQScores 1. Please set --printQScores and rerun.");
    if ((a.adjust_qs & 16) && !a.print_gl_err) die("--adjust-qs 16 requires --printGlError 1. Please set --printGlError 1 and rerun.");
    range(a.device_bgzf, 0, 1, "--device-bgzf");
    range(a.print_pileup, 0, 1, "-printPileup"); range(a.print_truth, 0, 1, "-printTruth"); range(a.print_bpe, 0, 1, "-printBasePickError");
    range(a.print_qs_err, 0, 1, "-printQsError"); range(a.print_gl_err, 0, 1, "-printGlError"); range(a.print_qscores, 0, 1, "-printQScores");
    if (a.print_gl_err && a.gl_model == 1)                                                                                              // io.cpp:993
        die("-> [-printGlError 1] Printing the error probability used in genotype likelihood calculations (-printGlError 1) is not supported with genotype likelihood model 1 (--gl-model 1).");
    if (a.gl_model == 1 && a.precise_gl) die("Precise genotype likelihood error (--precise-gl 1) is not supported with genotype likelihood model 1 (--gl-model 1).");
    if (a.error_qs == 0 && a.beta_variance >= 0) die("--beta-variance %e requires --error-qs 1 or 2.", a.beta_variance);
    if (a.error_qs != 0 && !(a.error_rate > 0)) die("--error-qs 1 or 2 requires --error-rate > 0 (found %f).", a.error_rate);
    if (a.error_qs != 0 && !(a.beta_variance > 0)) die("--error-qs 1 or 2 requires --beta-variance > 0 (found %e).", a.beta_variance);
    if (a.do_gvcf == 1) {                                                       // io.cpp:958-985
        if (!a.add_fmt_dp) die("[-doGVCF 1] -addFormatDP 1 is required for gVCF output. Please set -addFormatDP 1 and rerun.");
        if (a.rm_invar != 0) die("-> [-doGVCF 1] --rm-invar-sites 0 is required. Please set --rm-invar-sites 0 and rerun.");
        if (a.gvcf_dps_str.empty()) die("-> [-doGVCF 1] --gvcf-dps is required. Please set --gvcf-dps and rerun.");
        if (!(a.do_unobserved == 1 || a.do_unobserved == 2 || a.do_unobserved == 4 || a.do_unobserved == 5))
            die("-> [-doGVCF 1] Adding unobserved alleles is required for gVCF output. Please set -doUnobserved to 1 or 2 and rerun.");
        if (!a.add_pl) die("-> [-doGVCF 1] -addPL 1 is required for gVCF output. Please set -addPL 1 and rerun.");
        std::vector<std::string> parts; std::string cur;                          // gvcfData_init, bcf_utils.cpp:946-985
        for (char ch : a.gvcf_dps_str) { if (ch == ',') { parts.push_back(cur); cur.clear(); } else cur += ch; }
        parts.push_back(cur);
        for (auto& x : parts) { if (x.empty()) die("Could not parse --gvcf-dps %s", a.gvcf_dps_str.c_str()); const int d = atoi(x.c_str()); if (d < 1) die("Invalid DP range: %d", d); a.gvcf_dps.push_back(d); }
    } else if (!a.gvcf_dps_str.empty()) die("-> [--gvcf-dps] --gvcf-dps requires -doGVCF 1. Please set -doGVCF 1 and rerun.");
    if (a.output_mode != "v" && a.output_mode != "z" && a.output_mode != "u" && a.output_mode != "b")
        die("[Bad argument value: '--output-mode %s'] Allowed values are b, u, z, v", a.output_mode.c_str());
    if ((a.output_mode == "v" || a.output_mode == "z") && a.threads > 1)                      // io.cpp:1206-1210
        die("Multithreading is not supported for VCF output. Please set --threads 1 and rerun.");
    range(a.device_text, 0, 1, "--device-text");
    if (a.device_text) {                                        // (checked before any GPU work: nothing is written)
        if (a.output_mode != "v" && a.output_mode != "z") die("--device-text 1 formats VCF text: it needs -O v or -O z (found -O %s).", a.output_mode.c_str());
        if (a.do_gvcf) die("--device-text 1 is not supported with -doGVCF 1 (the gVCF blocker reads the FORMAT arrays of every site on the host); use --device-gvcf 1.");
        if (a.depth_inf) die("--device-text 1 is not supported with --depth inf (no tile is simulated).");
    }
    range(a.device_gvcf, 0, 1, "--device-gvcf");
    if (a.device_gvcf) {                                        // (checked before any GPU work: nothing is written)
        if (!a.do_gvcf) die("--device-gvcf 1 builds gVCF blocks: it needs -doGVCF 1.");
        if (a.output_mode != "v" && a.output_mode != "z" && a.device_bcf != 1)
            die("--device-gvcf 1 writes gVCF text: it needs -O v or -O z (found -O %s).", a.output_mode.c_str());
    }
    range(a.device_bcf, 0, 1, "--device-bcf");
    if (a.device_bcf) {                                         // (checked before any GPU work: nothing is written)
        if (a.output_mode != "u" && a.output_mode != "b") die("--device-bcf 1 encodes BCF records: it needs -O u or -O b (found -O %s).", a.output_mode.c_str());
        if (a.do_gvcf && !a.device_gvcf)
            die("--device-bcf 1 is not supported with -doGVCF 1 alone (the host blocker reads the FORMAT arrays of every site); add --device-gvcf 1.");
    }
    if (a.device_stream) {                                      // (checked before any GPU work: nothing is written)
        if (a.output_mode != "b" && a.output_mode != "z")
            die("--device-stream 1 assembles and compresses BGZF streams: it needs -O b or -O z (found -O %s).", a.output_mode.c_str());
        if (a.do_gvcf) die("--device-stream 1 is not supported with -doGVCF 1 (blocks carried across tiles are emitted by the host).");
        if (a.output_mode == "b" && !a.device_bcf) die("--device-stream 1 with -O b assembles the records --device-bcf 1 encodes: add --device-bcf 1.");
        if (a.output_mode == "z" && !a.device_text) die("--device-stream 1 with -O z assembles the records --device-text 1 formats: add --device-text 1.");
    }
    range(a.device_pileup, 0, 1, "--device-pileup");
    if (a.device_pileup) {                                      // (checked before any GPU work: nothing is written)
        if (!a.print_pileup) die("--device-pileup 1 formats the pileup of -printPileup 1: it needs -printPileup 1.");
        if (a.depth_inf) die("--device-pileup 1 is not supported with --depth inf (no tile is simulated, no pileup is written).");
    }
    if (a.seed == -1) { a.seed = (int)time(NULL); fprintf(stderr, "\n-> No seed was given. Setting the random seed to the randomly chosen value: %d\n", a.seed); }
    if (a.beta_sampler < 0) a.beta_sampler = (a.rng_mode == VGL_RNG_SERIAL) ? VGL_BETA_STD : VGL_BETA_RAND48;
    if (!a.depths_fn.empty()) {
        FILE* fp = fopen(a.depths_fn.c_str(), "r"); if (!fp) die("Could not open file: %s", a.depths_fn.c_str());
        double d; while (fscanf(fp, "%lf", &d) == 1) a.depths.push_back(d);
        fclose(fp);
    }
    if (!a.qs_bins_fn.empty()) {
        FILE* fp = fopen(a.qs_bins_fn.c_str(), "r"); if (!fp) die("Could not open file: %s", a.qs_bins_fn.c_str());
        int x, y, z; while (fscanf(fp, "%d,%d,%d", &x, &y, &z) == 3) { a.qs_bins.push_back(x); a.qs_bins.push_back(y); a.qs_bins.push_back(z); }
        fclose(fp);
    }
    return a;
}

// ---------------------------------------------------------------------------------------
// htslib kputd(): floats of VCF text.  0 -> "0"; outside [1e-4, 999999] -> "%g"; otherwise
// trunc(d*1e10) plus half a unit of the 6th significant digit, cut to 6 significant digits,
// trailing zeros removed.
static void put_float(std::string& s, float f) {
    uint32_t bits; memcpy(&bits, &f, 4);
    if (bits == VGL_FLOAT_MISSING_BITS) { s += '.'; return; }
    double d = f;
    if (isnan(d)) { s += "nan"; return; }
    if (d == 0) { s += signbit(d) ? "-0" : "0"; return; }
    if (d < 0) { s += '-'; d = -d; }
    char buf[64];
    if (!(d >= 0.0001 && d <= 999999)) { snprintf(buf, sizeof buf, "%g", d); s += buf; return; }
    uint64_t i = (uint64_t)(d * 10000000000LL);
    if (d < .0001) i += 0; else if (d < 0.001) i += 5; else if (d < 0.01) i += 50; else if (d < 0.1) i += 500;
    else if (d < 1) i += 5000; else if (d < 10) i += 50000; else if (d < 100) i += 500000; else if (d < 1000) i += 5000000;
    else if (d < 10000) i += 50000000; else if (d < 100000) i += 500000000; else i += 5000000000LL;
    char dig[32]; int n = snprintf(dig, sizeof dig, "%llu", (unsigned long long)i);   // d*1e10 as an integer
    std::string out;
    if (n <= 10) {                       // d < 1: "0." + leading zeros + 6 significant digits
        out = "0.";
        out.append(10 - n, '0');
        out.append(dig, n < 6 ? n : 6);
    } else {                             // integer part has n-10 digits; 6 significant digits in all
        const int ip = n - 10;
        out.append(dig, ip);
        if (ip < 6) { out += '.'; out.append(dig + ip, 6 - ip); }
    }
    if (out.find('.') != std::string::npos) {
        while (out.back() == '0') out.pop_back();
        if (out.back() == '.') out.pop_back();
    }
    s += out;
}

static void put_int(std::string& s, int32_t v) {
    if (v == VGL_INT32_MISSING) { s += '.'; return; }
    char buf[16]; snprintf(buf, sizeof buf, "%d", v); s += buf;
}

// ---------------------------------------------------------------------------------------
struct Rec {
    std::string chrom, id, qual, filt, info;
    long pos0;
    std::vector<std::string> alleles;
    std::vector<int8_t> gt;            // 2 per sample, allele index or -1
    std::vector<std::string> gt_str;   // GT tokens as written in the input (for -printTruth)
    char ref_char;
    const uint8_t* dev_row = nullptr;  // --device-input 1: the packed row the device parsed (Vcf::gt_rows), gt stays empty
    int32_t dev_sum = 0;               //                   and its allele sum
    int8_t in_status = -1;             // --dump-gt: VGL_VCFIN_OK / VGL_VCFIN_HOST of the line
};

// --device-input: how read_vcf is to parse the sample columns, and what it did (the [input] line of --verbose 1)
struct InputOpt {
    int device_input = 0, source = 0, device = 0, tile_sites = 4096; bool classify = false;
    int device_inflate = 0;                                  // --device-inflate 1: a BGZF file's members are inflated on `device`
    std::function<vgl_inflate_host*()> inflater;            // the host object, created beside the file read (waits for its creation; dies without a device)
};
struct InputStats {
    double t_read = 0, t_scan = 0, t_fixed = 0, t_dev = 0, t_host = 0; long lines_dev = 0, lines_host = 0; int64_t text_up = 0;
    // --device-inflate 1: members inflated on the device, compressed bytes sent up, inflated bytes received, why zlib read the file after all
    long members_dev = 0; int64_t inflate_up = 0, inflate_down = 0; const char* fallback = nullptr; double t_inflate = 0;
};

struct Vcf {
    std::vector<std::string> header;   // '##' lines
    std::vector<std::string> samples;
    std::map<std::string, long> contig_len;
    std::vector<Rec> recs;
    std::vector<uint8_t> gt_rows;      // --device-input 1: one row of packed true genotypes per record line (Rec::dev_row points here)
};

static void split(const std::string& s, char c, std::vector<std::string>& out) {
    out.clear(); size_t b = 0;
    while (true) { size_t e = s.find(c, b); if (e == std::string::npos) { out.push_back(s.substr(b)); break; } out.push_back(s.substr(b, e - b)); b = e + 1; }
}

// ---------------------------------------------------------------------------------------
// BCF 2.x input (raw or BGZF; zlib reads the gzip members): header text, then records decoded back
// into the same Rec the text reader fills -- QUAL / FILTER / INFO as VCF text, GT as allele indices.
struct BcfIn {
    std::vector<uint8_t> buf; size_t off = 0;
    std::map<int, std::string> dict, contig; std::map<std::string, int> info_is_flag;
    uint32_t u32() { if (off + 4 > buf.size()) die("truncated BCF record"); uint32_t v; memcpy(&v, &buf[off], 4); off += 4; return v; }
    void typed(int& type, int& n) {
        if (off >= buf.size()) die("truncated BCF record");
        const uint8_t b = buf[off++]; type = b & 15; n = b >> 4;
        if (n == 15) { int t2, n2; typed(t2, n2); std::vector<int32_t> v; ints(t2, n2, v); if (v.empty() || v[0] < 0) die("bad BCF vector length"); n = v[0]; }
    }
    void ints(int type, int n, std::vector<int32_t>& out) {          // missing -> INT32_MIN, end-of-vector -> INT32_MIN + 1
        const int w = type == 1 ? 1 : type == 2 ? 2 : type == 3 ? 4 : 0;
        if (!w) die("BCF: integer vector expected (type %d)", type);
        if (off + (size_t)w * n > buf.size()) die("truncated BCF record");
        out.clear();
        for (int i = 0; i < n; i++, off += w) {
            int32_t v;
            if (w == 1) { const int8_t x = (int8_t)buf[off]; v = x == -128 ? INT32_MIN : x == -127 ? INT32_MIN + 1 : x; }
            else if (w == 2) { int16_t x; memcpy(&x, &buf[off], 2); v = x == -32768 ? INT32_MIN : x == -32767 ? INT32_MIN + 1 : x; }
            else memcpy(&v, &buf[off], 4);
            out.push_back(v);
        }
    }
    std::string str(int n) { if (off + n > buf.size()) die("truncated BCF record"); std::string r((const char*)&buf[off], n); off += n; return r; }
    static std::string attr(const std::string& h, const char* key) {
        const std::string k = std::string(key) + "=";
        size_t a = h.find("<" + k); if (a == std::string::npos) a = h.find("," + k); if (a == std::string::npos) return "";
        a += k.size() + 1;
        return h.substr(a, h.find_first_of(",>", a) - a);
    }
};

static Vcf read_bcf(std::vector<uint8_t>&& raw, bool keep_gt_text) {
    BcfIn in; in.buf = std::move(raw);
    if (in.buf.size() < 9 || memcmp(in.buf.data(), "BCF\2", 4) != 0) die("not a BCF2 file");
    in.off = 5;
    const uint32_t l_text = in.u32();
    if (in.off + l_text > in.buf.size()) die("truncated BCF header");
    std::string text((const char*)&in.buf[in.off], l_text); in.off += l_text;
    while (!text.empty() && (text.back() == '\0' || text.back() == '\n')) text.pop_back();
    Vcf v; std::vector<std::string> lines, f; split(text, '\n', lines);
    int nd = 0, nc = 0; bool have_pass = false;
    for (const std::string& h : lines) if (h.compare(0, 10, "##FILTER=<") == 0 && BcfIn::attr(h, "ID") == "PASS") have_pass = true;
    if (!have_pass) { in.dict[0] = "PASS"; nd = 1; }
    for (const std::string& h : lines) {
        if (h.compare(0, 2, "##") != 0) { if (!h.empty() && h[0] == '#') { split(h, '\t', f); for (size_t i = 9; i < f.size(); i++) v.samples.push_back(f[i]); } continue; }
        v.header.push_back(h);
        const bool fil = h.compare(0, 10, "##FILTER=<") == 0, inf = h.compare(0, 8, "##INFO=<") == 0, fmt = h.compare(0, 10, "##FORMAT=<") == 0;
        const bool ctg = h.compare(0, 10, "##contig=<") == 0;
        if (!(fil || inf || fmt || ctg)) continue;
        const std::string id = BcfIn::attr(h, "ID"), idx_s = BcfIn::attr(h, "IDX");
        if (ctg) {
            const int idx = idx_s.empty() ? nc : atoi(idx_s.c_str());
            in.contig[idx] = id; nc = std::max(nc, idx + 1);
            const std::string len = BcfIn::attr(h, "length"); v.contig_len[id] = len.empty() ? -1 : atol(len.c_str());
            continue;
        }
        int idx = -1;
        for (auto& kv : in.dict) if (kv.second == id) idx = kv.first;
        if (idx < 0) idx = idx_s.empty() ? nd : atoi(idx_s.c_str());
        in.dict[idx] = id; nd = std::max(nd, idx + 1);
        if (inf) in.info_is_flag[id] = BcfIn::attr(h, "Type") == "Flag";
    }
    const size_t N = v.samples.size();
    std::vector<int32_t> iv; int type, n;
    while (in.off < in.buf.size()) {
        const uint32_t l_shared = in.u32(), l_indiv = in.u32();
        const size_t rec_end = in.off + (size_t)l_shared + l_indiv, shared_end = in.off + l_shared;
        if (rec_end > in.buf.size()) die("truncated BCF record");
        Rec r;
        const int32_t chrom = (int32_t)in.u32(); r.pos0 = (int32_t)in.u32(); (void)in.u32();
        const uint32_t qual = in.u32(), nai = in.u32(), nfs = in.u32();
        const int n_allele = nai >> 16, n_info = nai & 0xFFFF, n_fmt = nfs >> 24; const size_t n_sample = nfs & 0xFFFFFF;
        if (!in.contig.count(chrom)) die("BCF record with an undefined contig index %d", chrom);
        if (n_sample != N) die("Record at position %ld has %zu samples, the header names %zu samples.", r.pos0 + 1, n_sample, N);
        r.chrom = in.contig[chrom];
        if (qual == VGL_FLOAT_MISSING_BITS) r.qual = "."; else { float q; memcpy(&q, &qual, 4); put_float(r.qual, q); }
        in.typed(type, n); r.id = (type == 7) ? in.str(n) : "."; if (r.id.empty()) r.id = ".";
        for (int i = 0; i < n_allele; i++) { in.typed(type, n); if (type != 7) die("BCF: allele string expected"); r.alleles.push_back(in.str(n)); }
        if (r.alleles.empty() || r.alleles[0].empty()) die("Empty REF at position %ld.", r.pos0 + 1);
        r.ref_char = r.alleles[0][0];
        in.typed(type, n);
        if (type == 0 || n == 0) r.filt = "."; else { in.ints(type, n, iv); for (size_t i = 0; i < iv.size(); i++) { if (i) r.filt += ';'; if (!in.dict.count(iv[i])) die("BCF: undefined FILTER index"); r.filt += in.dict[iv[i]]; } }
        for (int i = 0; i < n_info; i++) {
            in.typed(type, n); in.ints(type, n, iv);
            if (iv.empty() || !in.dict.count(iv[0])) die("BCF: undefined INFO key");
            const std::string key = in.dict[iv[0]];
            if (!r.info.empty()) r.info += ';';
            r.info += key;
            in.typed(type, n);
            if (type == 0 || n == 0) continue;                              // flag
            r.info += '=';
            if (type == 7) r.info += in.str(n);
            else if (type == 5) { for (int k = 0; k < n; k++) { const uint32_t b = in.u32(); if (b == 0x7F800002u) continue; if (k) r.info += ','; float x; memcpy(&x, &b, 4); put_float(r.info, x); } }
            else { in.ints(type, n, iv); bool first = true; for (int32_t x : iv) { if (x == INT32_MIN + 1) continue; if (!first) r.info += ','; first = false; put_int(r.info, x); } }
        }
        if (r.info.empty()) r.info = ".";
        if (in.off != shared_end) die("BCF record: shared block length mismatch at position %ld", r.pos0 + 1);
        bool have_gt = false;
        r.gt.assign(2 * N, -1);
        for (int k = 0; k < n_fmt; k++) {
            in.typed(type, n); in.ints(type, n, iv);
            if (iv.empty() || !in.dict.count(iv[0])) die("BCF: undefined FORMAT key");
            const bool is_gt = in.dict[iv[0]] == "GT";
            in.typed(type, n);
            const size_t w = type == 1 ? 1 : type == 2 ? 2 : (type == 3 || type == 5) ? 4 : type == 7 ? 1 : 0;
            if (!is_gt) { if (in.off + w * n * N > in.buf.size()) die("truncated BCF record"); in.off += w * n * N; continue; }
            have_gt = true;
            for (size_t s = 0; s < N; s++) {
                in.ints(type, n, iv);
                int8_t a[2] = {-1, -1}; std::string txt;
                for (int j = 0; j < n && iv[j] != INT32_MIN + 1; j++) {
                    const int al = (iv[j] >> 1) - 1;
                    if (j < 2) a[j] = (int8_t)al;
                    if (keep_gt_text) { if (j) txt += (iv[j] & 1) ? '|' : '/'; if (al < 0) txt += '.'; else { char t[16]; snprintf(t, sizeof t, "%d", al); txt += t; } }
                }
                if (n == 1 || (n >= 2 && iv[1] == INT32_MIN + 1)) a[1] = a[0];     // haploid call: both alleles, as the text reader does
                r.gt[2 * s] = a[0]; r.gt[2 * s + 1] = a[1];
                if (keep_gt_text) r.gt_str.push_back(txt.empty() ? "." : txt);
            }
        }
        if (!have_gt) die("Could not find GT tag at position %ld.", r.pos0 + 1);
        in.off = rec_end;
        v.recs.push_back(std::move(r));
    }
    return v;
}

// keep_gt_text: the GT tokens as written are needed only by -printTruth
// The first nine columns of one record line [lb, le) -> Rec, the index of GT in FORMAT and the start of the sample columns.
// strict: exits on a line without ten columns or without GT; otherwise such a line returns false (r is then to be discarded).
static bool parse_fixed(const char* lb, const char* le, const bool strict, Rec& r, int& gti, const char*& samples) {
    const char* col_at[10]; int nc = 0; col_at[0] = lb;
    for (const char* q = lb; q < le && nc < 9; q++) if (*q == '\t') col_at[++nc] = q + 1;
    if (nc < 9) { if (!strict) return false; die("VCF record with fewer than 10 columns (a FORMAT/GT column is required)"); }
    auto col = [&](int k) { return std::string(col_at[k], (size_t)(col_at[k + 1] - 1 - col_at[k])); };
    std::vector<std::string> g, fmt;
    r.chrom = col(0); r.pos0 = atol(col(1).c_str()) - 1; r.id = col(2); r.qual = col(5); r.filt = col(6); r.info = col(7);
    const std::string ref = col(3), alt = col(4);
    r.alleles.push_back(ref);
    if (alt != ".") { split(alt, ',', g); for (auto& x : g) r.alleles.push_back(x); }
    if (ref.empty()) { if (!strict) return false; die("Empty REF at position %ld.", r.pos0 + 1); }
    r.ref_char = ref[0];
    split(col(8), ':', fmt);
    gti = -1; for (size_t i = 0; i < fmt.size(); i++) if (fmt[i] == "GT") gti = (int)i;
    if (gti < 0) { if (!strict) return false; die("Could not find GT tag at position %ld.", r.pos0 + 1); }
    samples = col_at[9];
    return true;
}

// The sample columns [p, le) of a record line -> Rec::gt (and the tokens as written)
static void parse_samples(const char* p, const char* le, const int gti, const size_t n_hdr, const bool keep_gt_text, Rec& r) {
    r.gt.assign(2 * n_hdr, -1);
    const char* const end = le;
    size_t s = 0;
    while (true) {                                       // p at the start of a sample column
        const char* ce = (const char*)memchr(p, '\t', (size_t)(end - p)); if (!ce) ce = end;
        if (s >= n_hdr) { s++; if (ce == end) break; p = ce + 1; continue; }
        const char* t = p;                               // the gti-th ':'-separated subfield; trailing ones may be dropped
        for (int k = 0; k < gti && t; k++) { t = (const char*)memchr(t, ':', (size_t)(ce - t)); if (t) t++; }
        const char* te = t ? (const char*)memchr(t, ':', (size_t)(ce - t)) : nullptr; if (t && !te) te = ce;
        int8_t a0 = -1, a1 = -1;
        if (t) {
            const char* sep = t; while (sep < te && *sep != '|' && *sep != '/') sep++;
            auto allele = [](const char* b, const char* e) -> int8_t { return (b == e || *b == '.') ? (int8_t)-1 : (int8_t)atoi(std::string(b, e).c_str()); };
            a0 = allele(t, sep);
            a1 = (sep == te) ? a0 : allele(sep + 1, te);
            if (keep_gt_text) r.gt_str.emplace_back(t, te);
        } else if (keep_gt_text) r.gt_str.emplace_back(".");
        r.gt[2 * s] = a0; r.gt[2 * s + 1] = a1;
        s++;
        if (ce == end) break;
        p = ce + 1;
    }
    if (s != n_hdr) die("Record at position %ld has %zu sample columns, the header names %zu samples.", r.pos0 + 1, s, n_hdr);
}

// one record line [lb, le) -> Rec (thread safe: records are parsed in parallel)
static void parse_record(const char* lb, const char* le, const size_t n_hdr, const bool keep_gt_text, Rec& r) {
    int gti; const char* p;
    parse_fixed(lb, le, true, r, gti, p);
    parse_samples(p, le, gti, n_hdr, keep_gt_text, r);
}

// --dump-gt: the status the device parser gives the sample columns [p, le) (include/vcfgl_hip.h: the plain grammar), on the host
static int classify_samples(const char* p, const char* le, const int gti, const int n_alleles, const size_t n_hdr) {
    size_t s = 0; bool plain = true;
    auto allele = [&](const char*& q, const char* te) {          // '.' or one or two digits below n_alleles
        if (q == te) return false;
        if (*q == '.') { q++; return true; }
        if (*q < '0' || *q > '9') return false;
        int v = *q++ - '0';
        if (q < te && *q >= '0' && *q <= '9') v = v * 10 + (*q++ - '0');
        return v < n_alleles;
    };
    while (true) {
        const char* ce = (const char*)memchr(p, '\t', (size_t)(le - p)); if (!ce) ce = le;
        const char* t = p;
        for (int k = 0; k < gti && t; k++) { t = (const char*)memchr(t, ':', (size_t)(ce - t)); if (t) t++; }
        if (t) {
            const char* te = (const char*)memchr(t, ':', (size_t)(ce - t)); if (!te) te = ce;
            const char* q = t;
            if (!allele(q, te)) plain = false;
            else if (q != te) { if (*q != '|' && *q != '/') plain = false; else { q++; if (!allele(q, te) || q != te) plain = false; } }
        }
        s++;
        if (ce == le) break;
        p = ce + 1;
    }
    return (plain && s == n_hdr) ? VGL_VCFIN_OK : VGL_VCFIN_HOST;
}

static int allele_to_int(const std::string& a);
static double now_s() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }

// make_site's allele table ra[] for a record, without its exits: false where make_site would refuse the record
static bool allele_table(const Rec& r, const int source, int8_t ra[5]) {
    for (int i = 0; i < 5; i++) ra[i] = -1;
    const int n = (int)r.alleles.size();
    if (n > 5 || (source == 0 && n > 2)) return false;
    for (int i = 0; i < n; i++) {
        if (source == 1) { const int x = r.alleles[i].empty() ? -1 : allele_to_int(r.alleles[i]); if (x == -1) return false; ra[i] = (int8_t)x; }
        else { const int x = (r.alleles[i].empty() ? 0 : r.alleles[i][0]) - '0'; if (x != 0 && x != 1) return false; ra[i] = (int8_t)x; }
    }
    return true;
}

// --device-input 1: the record lines' first nine columns on `threads` host threads, their sample columns on the device in batches of
// at most tile_sites lines (vgl_vcfin_host_*: one batch is copied up and parsed while the next is put together), and the host's own
// parser for every line the device hands back (VGL_VCFIN_HOST) or the fixed columns cannot describe -- its exits and messages are
// therefore those of --device-input 0.
static void parse_lines_device(const uint8_t* raw, const std::vector<std::pair<const char*, const char*>>& rec_lines, const size_t n_hdr,
                               const bool keep_gt_text, const int threads, const InputOpt& opt, Vcf& v, InputStats& st) {
    const int n = (int)rec_lines.size();
    const int N = (int)n_hdr;
    double t0 = now_s();
    std::vector<int64_t> lb((size_t)n), le((size_t)n);
    std::vector<int32_t> gti((size_t)n), nal((size_t)n);
    std::vector<int8_t> amap((size_t)n * 5);
    std::vector<uint8_t> sent((size_t)n, 0);
    vsink::parallel_for(n, threads, [&](int i) {
        Rec& r = v.recs[i];
        int g = -1; const char* p = nullptr;
        if (parse_fixed(rec_lines[i].first, rec_lines[i].second, false, r, g, p) && allele_table(r, opt.source, &amap[(size_t)i * 5])) {
            lb[i] = p - (const char*)raw; le[i] = rec_lines[i].second - (const char*)raw; gti[i] = g; nal[i] = (int32_t)r.alleles.size();
            sent[i] = 1;
        } else { r = Rec(); parse_record(rec_lines[i].first, rec_lines[i].second, n_hdr, keep_gt_text, r); r.in_status = VGL_VCFIN_HOST; }
    });
    st.t_fixed = now_s() - t0; t0 = now_s();
    const int TS = std::max(1, opt.tile_sites);
    const int nb = (n + TS - 1) / TS;
    // a batch: the sent lines among TS consecutive ones, and the text from the first one's sample columns to the last one's end
    struct Batch { std::vector<int> idx; int64_t t0 = 0, t1 = 0; };
    std::vector<Batch> batches((size_t)nb);
    int64_t max_text = 1; int max_lines = 1;
    for (int b = 0; b < nb; b++) {
        Batch& B = batches[b];
        for (int i = b * TS; i < std::min(n, (b + 1) * TS); i++) if (sent[i]) B.idx.push_back(i);
        if (B.idx.empty()) continue;
        B.t0 = lb[B.idx.front()]; B.t1 = le[B.idx.back()];
        max_text = std::max(max_text, B.t1 - B.t0); max_lines = std::max(max_lines, (int)B.idx.size());
    }
    v.gt_rows.resize((size_t)n * (size_t)N);
    std::vector<int> again;                                          // lines the device handed back
    vgl_vcfin_host* h = nullptr;
    if (vgl_vcfin_host_create(opt.device, N, max_lines, max_text, &h) != VGL_OK) die("--device-input 1: %s", vgl_last_error());
    std::vector<int64_t> blb[2], ble[2]; std::vector<int32_t> bg[2], bn[2]; std::vector<int8_t> bm[2];
    int32_t ticket[2] = {-1, -1};
    auto submit = [&](int b) {
        const Batch& B = batches[b]; const int k = b & 1; const size_t m = B.idx.size();
        blb[k].resize(m); ble[k].resize(m); bg[k].resize(m); bn[k].resize(m); bm[k].resize(m * 5);
        for (size_t j = 0; j < m; j++) {
            const int i = B.idx[j];
            blb[k][j] = lb[i] - B.t0; ble[k][j] = le[i] - B.t0; bg[k][j] = gti[i]; bn[k][j] = nal[i]; memcpy(&bm[k][j * 5], &amap[(size_t)i * 5], 5);
        }
        if (vgl_vcfin_host_submit(h, raw + B.t0, B.t1 - B.t0, (int32_t)m, blb[k].data(), ble[k].data(), bg[k].data(), bn[k].data(), bm[k].data(), &ticket[k]) != VGL_OK)
            die("--device-input 1: %s", vgl_last_error());
        st.text_up += m ? B.t1 - B.t0 : 0; st.lines_dev += (long)m;
    };
    auto retire = [&](int b) {
        const Batch& B = batches[b];
        const uint8_t* rows; const int32_t* sums; const int32_t* status;
        if (vgl_vcfin_host_wait(h, ticket[b & 1], &rows, &sums, &status) != VGL_OK) die("--device-input 1: %s", vgl_last_error());
        for (size_t j = 0; j < B.idx.size(); j++) {
            const int i = B.idx[j];
            if (status[j] != VGL_VCFIN_OK) { again.push_back(i); continue; }
            uint8_t* dst = &v.gt_rows[(size_t)i * (size_t)N];
            memcpy(dst, rows + j * (size_t)N, (size_t)N);
            v.recs[i].dev_row = dst; v.recs[i].dev_sum = sums[j]; v.recs[i].in_status = VGL_VCFIN_OK;
        }
    };
    for (int b = 0; b < nb; b++) { submit(b); if (b > 0) retire(b - 1); }
    if (nb > 0) retire(nb - 1);
    vgl_vcfin_host_destroy(h);
    st.t_dev = now_s() - t0; t0 = now_s();
    st.lines_host = (long)again.size();
    vsink::parallel_for((int)again.size(), threads, [&](int k) {
        const int i = again[k]; Rec& r = v.recs[i];
        r = Rec(); parse_record(rec_lines[i].first, rec_lines[i].second, n_hdr, keep_gt_text, r); r.in_status = VGL_VCFIN_HOST;
    });
    // -printTruth 1 writes the GT tokens as they stand in the input: collected on the host, as with --device-input 0
    if (keep_gt_text) vsink::parallel_for(n, threads, [&](int i) {
        Rec& r = v.recs[i];
        if (r.dev_row) { parse_samples((const char*)raw + lb[i], rec_lines[i].second, gti[i], n_hdr, true, r); r.gt.clear(); r.gt.shrink_to_fit(); }
    });
    st.t_host = now_s() - t0;
}

// keep_gt_text: the GT tokens as written are needed only by -printTruth.  The (decompressed) file is read whole,
// the header lines are taken in order and the record lines are parsed on `threads` threads.
// --device-inflate 1: the file as it lies on the disk, its members listed by vgl_bgzf_index and inflated on the device in batches of
// 512 (the compressor's batch: 32 MiB of output at most), two batches in flight.  false, with the reason in st.fallback, when the
// file is not a series of BGZF members or a member came back VGL_INFLATE_HOST: zlib then reads the whole file as without the flag,
// so that a damaged file gives what it gives today.  A device error ends the run.
static const int INFLATE_BATCH = 512;
static bool inflate_on_device(const std::string& fn, const InputOpt& opt, std::vector<uint8_t>& raw, InputStats& st) {
    std::vector<uint8_t> file;
    {
        FILE* f = fopen(fn.c_str(), "rb");
        if (!f) die("Could not open file: %s", fn.c_str());
        std::vector<uint8_t> chunk(1 << 22);
        size_t k;
        while ((k = fread(chunk.data(), 1, chunk.size(), f)) > 0) file.insert(file.end(), chunk.begin(), chunk.begin() + k);
        fclose(f);
    }
    vgl_inflate_host* h = opt.inflater();                 // (without a device the run ends here, whatever the file holds)
    const double t0 = now_s();
    const int64_t cap = (int64_t)file.size() / 28 + 1;
    std::vector<int64_t> begin((size_t)cap); std::vector<int32_t> csize((size_t)cap), isize((size_t)cap);
    int64_t n = 0;
    if (file.empty() || vgl_bgzf_index(file.data(), (int64_t)file.size(), cap, begin.data(), csize.data(), isize.data(), &n) != VGL_OK) {
        st.fallback = "the file is not a series of BGZF members"; st.t_inflate = now_s() - t0;
        return false;
    }
    int64_t total = 0;
    for (int64_t m = 0; m < n; m++) total += isize[(size_t)m];
    raw.resize((size_t)total);
    const int64_t n_batches = (n + INFLATE_BATCH - 1) / INFLATE_BATCH;
    int32_t ticket[2] = {0, 0};
    bool ok = true;
    int64_t out_at = 0;
    auto submit = [&](int64_t b) {
        const int64_t m0 = b * INFLATE_BATCH, m1 = std::min(n, m0 + INFLATE_BATCH);
        const int64_t lo = begin[(size_t)m0], hi = begin[(size_t)m1 - 1] + csize[(size_t)m1 - 1];
        std::vector<int64_t> rel((size_t)(m1 - m0));
        for (int64_t m = m0; m < m1; m++) rel[(size_t)(m - m0)] = begin[(size_t)m] - lo;
        if (vgl_inflate_host_submit(h, file.data() + lo, hi - lo, (int32_t)(m1 - m0), rel.data(), csize.data() + m0, isize.data() + m0, &ticket[b & 1]) != VGL_OK)
            die("--device-inflate 1: %s", vgl_last_error());
        st.inflate_up += hi - lo;
    };
    if (n_batches > 0) submit(0);
    for (int64_t b = 0; b < n_batches; b++) {
        if (b + 1 < n_batches) submit(b + 1);
        const uint8_t* out; int64_t out_n; const int32_t* status;
        if (vgl_inflate_host_wait(h, ticket[b & 1], &out, &out_n, &status) != VGL_OK) die("--device-inflate 1: %s", vgl_last_error());
        const int64_t m0 = b * INFLATE_BATCH, m1 = std::min(n, m0 + INFLATE_BATCH);
        for (int64_t m = m0; m < m1; m++) if (status[m - m0] != VGL_INFLATE_OK) ok = false;
        if (out_at + out_n > total) die("--device-inflate 1: a batch returned more bytes than its members' ISIZE fields hold");
        if (out_n > 0) memcpy(raw.data() + out_at, out, (size_t)out_n);
        out_at += out_n; st.inflate_down += out_n; st.members_dev += (long)(m1 - m0);
    }
    st.t_inflate = now_s() - t0;
    if (!ok) { st.fallback = "a member was left to the host (VGL_INFLATE_HOST)"; raw.clear(); return false; }
    return true;
}

static Vcf read_vcf(const std::string& fn, bool keep_gt_text, int threads, const InputOpt& opt = InputOpt(), InputStats* stats = nullptr) {
    InputStats st; double t0 = now_s();
    std::vector<uint8_t> raw;
    if (!opt.device_inflate || !inflate_on_device(fn, opt, raw, st)) {
        gzFile fp = gzopen(fn.c_str(), "r");               // plain text, gzip / BGZF, or BCF inside either
        if (!fp) die("Could not open file: %s", fn.c_str());
        gzbuffer(fp, 1 << 20);
        std::vector<uint8_t> chunk(1 << 22);
        int k;
        while ((k = gzread(fp, chunk.data(), (unsigned)chunk.size())) > 0) raw.insert(raw.end(), chunk.begin(), chunk.begin() + k);
        gzclose(fp);
    }
    if (raw.size() >= 3 && !memcmp(raw.data(), "BCF", 3)) {
        if (opt.device_input) die("--device-input 1 is not supported with BCF input (its genotypes are binary already: there is no text to parse).");
        st.t_read = now_s() - t0;
        if (stats) *stats = st;
        return read_bcf(std::move(raw), keep_gt_text);
    }
    st.t_read = now_s() - t0; t0 = now_s();
    Vcf v;
    std::vector<std::string> f;
    std::vector<std::pair<const char*, const char*>> rec_lines;
    const char* p = (const char*)raw.data(); const char* const end = p + raw.size();
    while (p < end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        const char* le = nl ? nl : end;
        if (le > p) {
            if (le - p >= 2 && p[0] == '#' && p[1] == '#') {
                const std::string line(p, le);
                v.header.push_back(line);
                if (line.compare(0, 10, "##contig=<") == 0) {
                    size_t a = line.find("ID="), l = line.find("length=");
                    if (a != std::string::npos) {
                        std::string id = line.substr(a + 3, line.find_first_of(",>", a) - a - 3);
                        v.contig_len[id] = (l != std::string::npos) ? atol(line.c_str() + l + 7) : -1;
                    }
                }
            } else if (p[0] == '#') { split(std::string(p, le), '\t', f); for (size_t i = 9; i < f.size(); i++) v.samples.push_back(f[i]); }
            else rec_lines.emplace_back(p, le);
        }
        p = nl ? nl + 1 : end;
    }
    st.t_scan = now_s() - t0; t0 = now_s();
    v.recs.resize(rec_lines.size());
    const size_t n_hdr = v.samples.size();
    if (opt.device_input && n_hdr > 0) parse_lines_device(raw.data(), rec_lines, n_hdr, keep_gt_text, threads, opt, v, st);
    else {
        vsink::parallel_for((int)rec_lines.size(), threads, [&](int i) {
            Rec& r = v.recs[i];
            if (!opt.classify) { parse_record(rec_lines[i].first, rec_lines[i].second, n_hdr, keep_gt_text, r); return; }
            int gti; const char* sp;
            parse_fixed(rec_lines[i].first, rec_lines[i].second, true, r, gti, sp);
            parse_samples(sp, rec_lines[i].second, gti, n_hdr, keep_gt_text, r);
            r.in_status = (int8_t)classify_samples(sp, rec_lines[i].second, gti, (int)r.alleles.size(), n_hdr);
        });
        st.t_host = now_s() - t0; st.lines_host = (long)rec_lines.size();
    }
    if (stats) *stats = st;
    return v;
}

// allele_char_to_int, vcfgl.cpp:20-50
static int allele_to_int(const std::string& a) {
    if (a.size() > 1) return (a == "<*>" || a == "<NON_REF>") ? 4 : -1;
    switch (a[0]) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return -1; }
}

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

// page-locked host array (vgl_host_alloc): grows, never shrinks
template <class T> struct PBuf {
    T* p = nullptr; size_t n = 0;
    static int& device() { static thread_local int d = -1; return d; }   // >= 0: place the memory for DMA from that device (vgl_host_alloc_on)
    void resize(size_t m) {
        if (m <= n) return;
        if (p) vgl_host_free(p);
        p = (T*)(device() >= 0 ? vgl_host_alloc_on(device(), m * sizeof(T)) : vgl_host_alloc(m * sizeof(T)));
        if (!p) die("%s", vgl_last_error());
        n = m;
    }
    T* data() { return p; }
    const T* data() const { return p; }
    T& operator[](size_t i) { return p[i]; }
    const T& operator[](size_t i) const { return p[i]; }
    PBuf() = default; PBuf(const PBuf&) = delete; PBuf& operator=(const PBuf&) = delete;
    ~PBuf() { if (p) vgl_host_free(p); }
};

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
            dp.assign(sv->dp, sv->dp + sv->N);
            const int nG = sv->n_alleles * (sv->n_alleles + 1) / 2;
            pl.assign((size_t)sv->N * nG, 0);
            pl.assign(sv->pl, sv->pl + (size_t)sv->N * nG);                 // sample-major, like the block's own array
            qsum.clear(); if (sv->qs) qsum.assign(sv->qs, sv->qs + sv->n_alleles);
            chrom = *sv->chrom; start_pos = sv->pos0; alleles = sv->alleles; min_dp = mdp; current_dpr = dp_range;
        } else {
            if (min_dp > mdp) min_dp = mdp;
            for (int s = 0; s < sv->N; ++s) if (dp[s] > sv->dp[s]) dp[s] = sv->dp[s];
            if (sv->n_alleles != 2 || pl.size() != (size_t)sv->N * 3) die("Unexpected number of PL values: %d", sv->N * sv->n_alleles * (sv->n_alleles + 1) / 2);
            for (int s = 0; s < sv->N; ++s) {
                const int32_t p1 = sv->pl[(size_t)3 * s + 1], p2 = sv->pl[(size_t)3 * s + 2];
                if (pl[3 * s + 1] > p1) { pl[3 * s + 1] = p1; pl[3 * s + 2] = p2; }
                else if (pl[3 * s + 1] == p1 && pl[3 * s + 2] > p2) pl[3 * s + 2] = p2;
            }
        }
        end_pos = sv->pos0;
        return NO_WRITE;
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

// ---------------------------------------------------------------------------------------
int main(int argc, char** argv) {
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
        // test hook of the input parser: --dump-gt <file> <source 0|1> <device-input 0|1> prints per record line "pos status allelesum row":
        // the row make_site hands to the tile calls in hex, the status of the line (VGL_VCFIN_*: 1 = outside the device parser's plain
        // grammar), through the host parser (0, no GPU needed) or the device parser (1)
        Args a; a.source = atoi(argv[3]);
        InputOpt opt; opt.device_input = atoi(argv[4]); opt.source = a.source; opt.classify = true; opt.tile_sites = 256;
        if (a.source < 0 || a.source > 1 || opt.device_input < 0 || opt.device_input > 1) die("--dump-gt <file> <source 0|1> <device-input 0|1>");
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
    Args a = parse_args(argc, argv);
    if (a.device_input) {                                       // (checked before any file of the run exists, the .arg file included)
        gzFile fp = gzopen(a.in_fn.c_str(), "r"); char magic[3] = {0, 0, 0};
        if (!fp) die("Could not open file: %s", a.in_fn.c_str());
        const int k = gzread(fp, magic, 3); gzclose(fp);
        if (k == 3 && !memcmp(magic, "BCF", 3)) die("--device-input 1 is not supported with BCF input (its genotypes are binary already: there is no text to parse).");
    }
    RunLog runlog; runlog.open(a);
    // --verbose 1: wall-clock seconds per stage on stderr at the end
    double t_stage[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};          // read, sites, context, waiting for the device, encode, write, tile buffers (page-locked), teardown, pileup
    auto now = []() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; };
    double t_mark = now();
    auto lap = [&](int k) { const double t = now(); t_stage[k] += t - t_mark; t_mark = t; };
    // host threads for parsing and record encoding: --encode-threads, else --threads when given, else up to 8 of the
    // machine's threads -- the bytes written do not depend on it
    int enc_threads = a.enc_threads > 0 ? a.enc_threads : a.threads;
    if (a.enc_threads <= 0 && !a.threads_given) { const unsigned hc = std::thread::hardware_concurrency(); enc_threads = (int)std::max(1u, std::min(8u, hc)); }
    // the HIP runtime initialises (about 0.07 s) while the input is read and parsed
    std::thread hip_warm;
    // (on the first device the run selected: a primary context on GPU 0 would otherwise be created for a run that never uses it;
    //  a failure here is not swallowed for good -- vgl_ctx_create on the same device reports it below)
    const int warm_dev = a.devices.empty() ? a.device : a.devices[0];
    const int bgzf_dev = a.device_bgzf ? warm_dev : -1;         // --device-bgzf 1: the run's first device compresses every BGZF stream
    // --device-inflate 1: the inflater's page-locked staging and device buffers are made on that thread too, while the file is read
    vgl_inflate_host* inflater = nullptr; int inflater_rc = VGL_OK; std::string inflater_err;
    const bool want_inflater = a.device_inflate == 1;
    if (!a.depth_inf) hip_warm = std::thread([warm_dev, want_inflater, &inflater, &inflater_rc, &inflater_err] {
        vgl_host_free(vgl_host_alloc_on(warm_dev, 4096));
        if (want_inflater && (inflater_rc = vgl_inflate_host_create(warm_dev, INFLATE_BATCH, &inflater)) != VGL_OK) inflater_err = vgl_last_error();
    });
    InputOpt in_opt; in_opt.device_inflate = a.device_inflate;
    in_opt.inflater = [&]() -> vgl_inflate_host* {
        if (hip_warm.joinable()) hip_warm.join();
        if (inflater_rc != VGL_OK || !inflater) die("--device-inflate 1: %s", inflater_err.c_str());
        return inflater;
    };
    in_opt.device_input = a.device_input; in_opt.source = a.source; in_opt.device = warm_dev; in_opt.tile_sites = a.tile_sites > 0 ? a.tile_sites : 4096;
    InputStats in_stats;
    Vcf vcf = read_vcf(a.in_fn, a.print_truth != 0, enc_threads, in_opt, &in_stats);
    if (hip_warm.joinable()) hip_warm.join();
    if (inflater) { vgl_inflate_host_destroy(inflater); inflater = nullptr; }
    lap(0);
    const int N = (int)vcf.samples.size();
    if (N <= 0) die("no samples in %s", a.in_fn.c_str());
    if (!a.depths.empty() && (int)a.depths.size() != N) die("--depths-file must hold one depth per sample (%zu given, %d samples)", a.depths.size(), N);
    const char mode = a.output_mode[0];
    const std::string ext = mode == 'v' ? ".vcf" : mode == 'z' ? ".vcf.gz" : ".bcf";
    // binary output needs every contig / FILTER / INFO key of the records defined in the header (exploded sites carry the
    // contig of an input record)
    auto complete_header = [&](std::vector<std::string>& hdr) {
        if (mode != 'u' && mode != 'b') return;
        std::vector<std::string> contigs, filters, keys, tmp;
        auto add = [](std::vector<std::string>& v, const std::string& x) { if (!x.empty() && std::find(v.begin(), v.end(), x) == v.end()) v.push_back(x); };
        for (const Rec& r : vcf.recs) {
            add(contigs, r.chrom);
            split(r.filt, ';', tmp); for (auto& f : tmp) add(filters, f);
            if (r.info != ".") { split(r.info, ';', tmp); for (auto& kv : tmp) add(keys, kv.substr(0, kv.find('='))); }
        }
        vsink::Sink::define_missing(hdr, contigs, filters, keys);
    };
    SiteStream stream(a, vcf, N);
    vsink::Sink truth_sink; truth_sink.text_float = put_float;
    if (a.print_truth) {                                 // written as the sites go by (vcfgl.cpp:1518,1548,1607)
        std::vector<std::string> hdr = vcf.header;
        hdr.push_back("##source=vcfgl_hip"); hdr.push_back("##source=" + a.command);
        complete_header(hdr);
        truth_sink.open(a.out_prefix + ".truth" + ext, mode, hdr, vcf.samples, 1, bgzf_dev);
        stream.truth = &truth_sink;
    }
    size_t n_sites_total = 0;

    if (a.depth_inf) {                                   // simulate_record_true_values, vcfgl.cpp:1089-1262
        vsink::Sink out; out.text_float = put_float;
        std::vector<std::string> hdr;
        for (const std::string& h : vcf.header) if (h.find("##FORMAT=<ID=GT,") == std::string::npos) hdr.push_back(h);
        hdr.push_back("##source=vcfgl_hip"); hdr.push_back("##source=" + a.command);
        if (a.add_gl) hdr.push_back("##FORMAT=<ID=GL,Number=G,Type=Float,Description=\"log10 genotype likelihoods, best = 0\">");
        if (a.add_gp) hdr.push_back("##FORMAT=<ID=GP,Number=G,Type=Float,Description=\"Genotype probabilities\">");
        if (a.add_pl) hdr.push_back("##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods\">");
        complete_header(hdr);
        out.open(a.out_prefix + ext, mode, hdr, vcf.samples, 1, bgzf_dev);
        const bool explode_acgt = a.do_unobserved >= 3;
        const bool add_unobs = (a.do_unobserved == 1 || a.do_unobserved == 2 || a.do_unobserved == 4 || a.do_unobserved == 5);
        const char* nonref = (a.do_unobserved == 1 || a.do_unobserved == 4) ? "<*>" : "<NON_REF>";
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
            for (int i = 0; i < n_acgt; i++) { idx_of[order[i]] = (int)al.size(); al.push_back(std::string(1, "ACGT"[order[i]])); }
            if (add_unobs) al.push_back(nonref);
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
        return 0;
    }

    vgl_params p; memset(&p, 0, sizeof p);
    p.abi_version = VGL_ABI_VERSION; p.out_layout = VGL_LAYOUT_SAMPLE_MAJOR; p.seed = a.seed; p.n_samples = N; p.rng_mode = a.rng_mode; p.beta_sampler = a.beta_sampler;
    p.depth = a.depth; p.depths = a.depths.empty() ? nullptr : a.depths.data();
    p.error_rate = a.error_rate; p.error_qs = a.error_qs; p.beta_variance = a.beta_variance; p.gl_model = a.gl_model;
    p.gl1_theta = a.gl1_theta; p.precise_gl = a.precise_gl; p.adjust_qs = a.adjust_qs; p.adjust_by = a.adjust_by;
    p.n_qs_bins = (int)a.qs_bins.size() / 3; p.qs_bins = a.qs_bins.empty() ? nullptr : a.qs_bins.data(); p.i16_mapq = a.i16_mapq;
    p.do_unobserved = a.do_unobserved; p.rm_invar_sites = a.rm_invar; p.rm_empty_sites = a.rm_empty; p.do_gvcf = a.do_gvcf;
    p.add_gl = a.add_gl; p.add_gp = a.add_gp; p.add_pl = a.add_pl; p.add_i16 = a.add_i16; p.add_qs = a.add_qs;
    p.add_fmt_dp = a.add_fmt_dp; p.add_info_dp = a.add_info_dp; p.add_fmt_ad = a.add_fmt_ad; p.add_info_ad = a.add_info_ad;
    p.add_fmt_adf = a.add_fmt_adf; p.add_info_adf = a.add_info_adf; p.add_fmt_adr = a.add_fmt_adr; p.add_info_adr = a.add_info_adr;
    int TS = a.tile_sites > 0 ? a.tile_sites : 4096;
    const bool dpile = a.device_pileup != 0;                   // --device-pileup 1: the pileup's sample columns come from the device
    const bool dbcf = a.device_bcf != 0;                       // --device-bcf 1: the FORMAT part of BCF records comes from the device
    // per-read dump rows: the library's own staging capacity (vgl_host.cpp: depth + 8 sqrt(depth) + 16)
    double dmax = a.depth; for (double d : a.depths) dmax = std::max(dmax, d); if (!(dmax >= 0)) dmax = 0;
    const int pile_cap = (((int)ceil(dmax + 8.0 * sqrt(dmax) + 16.0)) + 3) & ~3;
    if ((a.print_pileup && !dpile) || a.print_qs_err || a.print_gl_err || a.print_qscores)      // per-read dumps: bounded host / device staging
        TS = std::max(1, std::min(TS, (int)((64u << 20) / ((size_t)1024 * (size_t)std::max(N, 1)) + 1)));
    else if (dpile) {                                           // the pileup text of a tile: at most 256 MiB per ring entry (two per device)
        const int64_t per_site = vgl_pileup_bound(N, 1, pile_cap);
        TS = std::max(1, (int)std::min<int64_t>(TS, (int64_t)(256u << 20) / std::max<int64_t>(per_site, 1)));
    }
    // ---- devices: one context and one host thread per GPU; tiles are dealt to them round robin and come back to the writer
    //      (this thread) in site order.  Every value depends only on the absolute site index (VGL_RNG_TILE), so the file does
    //      not depend on the number of devices.  VGL_RNG_SERIAL consumes its streams in call order: one device.
    std::vector<int> devices = a.devices.empty() ? std::vector<int>{a.device} : a.devices;
    if (devices.size() > 1 && a.rng_mode == VGL_RNG_SERIAL) die("--devices: --rng-mode 1 (the reference's serial draw order) does not shard; use one device");
    const int D = (int)devices.size();
    std::vector<vgl_ctx*> ctxs(D, nullptr);
    t_mark = now();
    for (int d = 0; d < D; d++) if (vgl_ctx_create(&p, devices[d], TS, &ctxs[d]) != VGL_OK) die("%s", vgl_last_error());
    if (a.gt_disc) for (int d = 0; d < D; d++) if (vgl_ctx_discordance(ctxs[d], 1) != VGL_OK) die("--gt-discordance 1: %s", vgl_last_error());
    lap(2);
    const int A = vgl_max_alleles(&p), G = vgl_max_genotypes(&p);
    const bool rec0 = a.records == 0;                         // --records 0: no record file, no FORMAT array back; the tiles are simulated and tallied

    // ---- output header (set_hdr, bcf_utils.cpp:511-615): input header minus FORMAT/GT, plus our tags
    vsink::Sink out; out.text_float = put_float;
    if (!rec0) {
        std::vector<std::string> hdr;
        char hb[128];
        for (const std::string& h : vcf.header) if (h.find("##FORMAT=<ID=GT,") == std::string::npos) hdr.push_back(h);
        snprintf(hb, sizeof hb, "##source=vcfgl_hip (libvcfgl_hip ABI %d, gfx950)", vgl_abi_version()); hdr.push_back(hb);
        hdr.push_back("##source=" + a.command);
        if (a.do_unobserved == 1 || a.do_unobserved == 4) hdr.push_back("##ALT=<ID=*,Description=\"Any other alternative allele (unobserved)\">");
        if (a.do_unobserved == 2 || a.do_unobserved == 5) hdr.push_back("##ALT=<ID=NON_REF,Description=\"Any other alternative allele (unobserved)\">");
        if (a.do_gvcf) { hdr.push_back("##INFO=<ID=END,Number=1,Type=Integer,Description=\"Last position of the non-variant block\">");
                         hdr.push_back("##INFO=<ID=MIN_DP,Number=1,Type=Integer,Description=\"Smallest per-sample depth within the block\">"); }
        if (a.add_fmt_dp) hdr.push_back("##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Simulated read depth of the sample\">");
        if (a.add_info_dp) hdr.push_back("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Read depth summed over samples\">");
        if (a.add_gl) hdr.push_back("##FORMAT=<ID=GL,Number=G,Type=Float,Description=\"log10 genotype likelihoods, best = 0\">");
        if (a.add_pl) hdr.push_back("##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods\">");
        if (a.add_gp) hdr.push_back("##FORMAT=<ID=GP,Number=G,Type=Float,Description=\"Genotype probabilities\">");
        if (a.add_qs) hdr.push_back("##INFO=<ID=QS,Number=R,Type=Float,Description=\"Normalised per-allele base quality sum\">");
        if (a.add_i16) hdr.push_back("##INFO=<ID=I16,Number=16,Type=Float,Description=\"bcftools call auxiliary tag\">");
        if (a.add_fmt_ad) hdr.push_back("##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Allelic depths\">");
        if (a.add_fmt_adf) hdr.push_back("##FORMAT=<ID=ADF,Number=R,Type=Integer,Description=\"Allelic depths, forward strand\">");
        if (a.add_fmt_adr) hdr.push_back("##FORMAT=<ID=ADR,Number=R,Type=Integer,Description=\"Allelic depths, reverse strand\">");
        if (a.add_info_ad) hdr.push_back("##INFO=<ID=AD,Number=R,Type=Integer,Description=\"Total allelic depths\">");
        if (a.add_info_adf) hdr.push_back("##INFO=<ID=ADF,Number=R,Type=Integer,Description=\"Total allelic depths, forward strand\">");
        if (a.add_info_adr) hdr.push_back("##INFO=<ID=ADR,Number=R,Type=Integer,Description=\"Total allelic depths, reverse strand\">");
        complete_header(hdr);
        // BGZF compression threads: --threads as in the reference; when it is not given, up to 8 (same bytes either way)
        out.open(a.out_prefix + ext, mode, hdr, vcf.samples, a.threads_given ? a.threads : (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency())), bgzf_dev);
    }
    int n_fmt = 0;                                              // FORMAT fields of a simulated record
    if (dbcf) {                                                 // dictionary ids of the FORMAT keys: the device writes them as typed keys
        const char* keys[7] = {"DP", "GL", "PL", "GP", "AD", "ADF", "ADR"};
        const int on[7] = {a.add_fmt_dp, a.add_gl, a.add_pl, a.add_gp, a.add_fmt_ad, a.add_fmt_adf, a.add_fmt_adr};
        int32_t ids[7];
        for (int k = 0; k < 7; k++) { ids[k] = on[k] ? out.key_id(keys[k]) : 0; n_fmt += on[k] ? 1 : 0; }
        for (int d = 0; d < D; d++) if (vgl_ctx_bcf_keys(ctxs[d], ids, 7) != VGL_OK) die("--device-bcf 1: %s", vgl_last_error());
    }
    FILE* pile_fp = nullptr; vsink::Bgzf pile;            // the reference writes the pileup through htslib's BGZF (vcfgl.cpp:1776-1783)
    if (a.print_pileup) {
        pile_fp = fopen((a.out_prefix + ".pileup.gz").c_str(), "wb"); if (!pile_fp) die("Could not open pileup output");
        pile.open(pile_fp, 1, bgzf_dev);
    }
    // ---- TSV lines on stdout (vcfgl.cpp:430-435, 533-554, 1745-1755)
    int pre_q = -1, pre_adjq = -1;                                              // preCalc->qScore / adj_qScore
    if (a.print_bpe && a.error_qs != 1) printf("base_pick_error_prob\tNA\tNA\tNA\tNA\t%f\n", a.error_rate);   // io.cpp:1089-1100
    if (a.error_qs != 2) {
        host_errprob_to_qs(a, a.error_rate, pre_q, pre_adjq);
        if (a.print_gl_err) printf("gl_error_prob\tNA\tNA\tNA\tNA\t%f\n", a.precise_gl ? a.error_rate : host_qs_to_errprob((a.adjust_qs & 1) ? pre_adjq : pre_q));
        if (a.print_qs_err) printf("qs_error_prob\tNA\tNA\tNA\tNA\t%f\n", a.error_rate);
        if (a.print_qscores) printf("qs\tNA\tNA\tNA\tNA\t%d\n", a.adjust_qs ? pre_adjq : pre_q);
    }
    const bool dump_reads = a.error_qs == 2 && (a.print_qs_err || a.print_gl_err || a.print_qscores);
    const bool want_errp = dump_reads || (a.error_qs == 2 && pile_fp && !dpile && (a.adjust_qs & 4));
    const bool dump_pick = a.error_qs == 1 && a.print_bpe;
    const char* nonref = (a.do_unobserved == 1 || a.do_unobserved == 4) ? "<*>" : "<NON_REF>";

    // ---- tile buffers (host side of vgl_tile_out): only what this run prints is requested from the device
    // --device-text 1: the FORMAT arrays stay on the device (formatted there), DP comes back only for the pileup / per-read listings
    // --device-bcf 1: the same two paths for -O u / -O b -- the tile's FORMAT part comes back as BCF typed vectors (vgl_ctx_bcf_keys)
    const bool dtext = a.device_text != 0 || (dbcf && !a.do_gvcf);
    // --device-gvcf 1: the same for -doGVCF 1; the blocks are built on the device, the FORMAT arrays stay there
    const bool dgvcf = a.device_gvcf != 0;
    // --device-pileup 1: the read dump and DP stay on the device (the pileup's sample columns come back as text)
    const bool want_dp = !rec0 && ((a.add_fmt_dp && !dtext && !dgvcf) || (a.do_gvcf && !dgvcf) || (pile_fp && !dpile) || dump_reads);
    struct TileBufs {
        int ns = 0; int64_t t0 = 0; int dev = 0;
        std::vector<SiteMeta> meta; std::vector<uint8_t> gt;
        // outputs live in page-locked memory (vgl_host_alloc): the device writes them by DMA while the next tile is computed
        PBuf<uint8_t> reads;
        PBuf<int32_t> st, na, nobs, idp, iad, iadf, iadr, dp, pl, ad, adf, adr;
        PBuf<int8_t> a2b; PBuf<float> qs, i16, gl, gp; PBuf<double> errp, pick;
        PBuf<uint8_t> text; PBuf<int64_t> toff; int64_t text_cap = 0;      // --device-text 1: the tile's sample columns and site offsets
        // --device-stream 1: the sample columns stay in body buffer `sbuf` of the device's stream handle; the heads of the tile's records
        // back to back and their offsets go up; sticket: the handle's ticket while the tile's members are on their way
        int sbuf = 0; int32_t sticket = -1; std::string heads; std::vector<int64_t> hoff;
        // --device-gvcf 1: contig id and position per site (in), the items, block offsets and the first / last block's aggregates (out)
        std::vector<int32_t> contig; std::vector<int64_t> pos0;
        PBuf<int32_t> gitems, fdp, fpl, ldp, lpl; PBuf<int64_t> boff; vgl_gvcf_tile g;
        PBuf<uint8_t> ptext; PBuf<int64_t> poff; vgl_pileup_tile pt;      // --device-pileup 1: the tile's pileup columns and site offsets
        vgl_tile_out o;
        std::mutex m; std::condition_variable cv; bool done = false;
    };
    const size_t E = (size_t)TS * N;
    const bool dstream = a.device_stream != 0;                  // --device-stream 1: records assembled and compressed where the tile was simulated
    // tiles in flight: two per device.  --device-stream 1: three -- an entry stays busy until its members are written, one tile behind
    // the writer, and with two the device would wait for the writer before every other tile
    const int R = (dstream ? 3 : 2) * D;
    // the stream handles (one per device) are created once the contexts know what a tile's bodies can take (below)
    std::vector<vgl_stream_host*> hstream(D, nullptr);
    std::vector<std::unique_ptr<TileBufs>> ring(R);
    // An entry's buffers are page-locked when the entry is first used (about 0.04 s per 250 MB): the second entry of a device is
    // prepared while the device already works on the first tile
    auto alloc_entry = [&](size_t ri) {
        auto& up = ring[ri];
        if (up) return;
        up.reset(new TileBufs());
        TileBufs& B = *up;
        // ring entry ri only ever serves device ri % D (tiles are dealt round robin, two entries per device): its page-locked
        // buffers are placed next to that device
        const int dev_of_entry = devices[ri % (size_t)D];
        PBuf<uint8_t>::device() = dev_of_entry; PBuf<int32_t>::device() = dev_of_entry; PBuf<int8_t>::device() = dev_of_entry;
        PBuf<float>::device() = dev_of_entry; PBuf<double>::device() = dev_of_entry; PBuf<int64_t>::device() = dev_of_entry;
        B.meta.resize(TS); B.gt.resize(E);
        B.st.resize(TS); B.na.resize(TS); B.nobs.resize(TS); B.a2b.resize((size_t)TS * 5);
        memset(&B.o, 0, sizeof B.o);
        B.o.site_status = B.st.data(); B.o.n_alleles = B.na.data(); B.o.n_alleles_obs = B.nobs.data(); B.o.alleles2acgt = B.a2b.data();
        if (rec0) return;                                        // (the per-site status and alleles above: a few bytes per site, for the run's summary)
        B.idp.resize(TS); B.o.info_dp = B.idp.data();           // also tells which sites reach the read loop (TSV dumps)
        if (a.add_info_ad) { B.iad.resize((size_t)TS * A); B.o.info_ad = B.iad.data(); }
        if (a.add_info_adf) { B.iadf.resize((size_t)TS * A); B.o.info_adf = B.iadf.data(); }
        if (a.add_info_adr) { B.iadr.resize((size_t)TS * A); B.o.info_adr = B.iadr.data(); }
        if (a.add_qs) { B.qs.resize((size_t)TS * A); B.o.qs = B.qs.data(); }
        if (a.add_i16) { B.i16.resize((size_t)TS * 16); B.o.i16 = B.i16.data(); }
        if (want_dp) { B.dp.resize(E); B.o.fmt_dp = B.dp.data(); }
        memset(&B.pt, 0, sizeof B.pt);
        if (dpile) {
            const int64_t cap = vgl_ctx_pileup_bound(ctxs[ri % (size_t)D], TS);
            if (cap < 0) die("--device-pileup 1: %s", vgl_last_error());
            B.ptext.resize((size_t)std::max<int64_t>(cap, 1)); B.poff.resize((size_t)TS + 1);
            B.pt.text = B.ptext.data(); B.pt.text_cap = cap; B.pt.offsets = B.poff.data();
        }
        if (dtext) {
            B.text_cap = vgl_ctx_text_bound(ctxs[ri % (size_t)D], TS);
            if (B.text_cap < 0) die("%s 1: %s", dbcf ? "--device-bcf" : "--device-text", vgl_last_error());
            B.toff.resize((size_t)TS + 1);
            if (dstream) { B.sbuf = (int)(ri / (size_t)D); B.hoff.resize((size_t)TS + 1); return; }     // (B.text is not allocated: the bodies stay on the device)
            B.text.resize((size_t)std::max<int64_t>(B.text_cap, 1));
            return;
        }
        if (dgvcf) {
            B.text_cap = vgl_ctx_gvcf_text_bound(ctxs[ri % (size_t)D], TS);
            if (B.text_cap < 0) die("--device-gvcf 1: %s", vgl_last_error());
            B.text.resize((size_t)std::max<int64_t>(B.text_cap, 1)); B.toff.resize((size_t)TS + 1); B.boff.resize((size_t)TS + 1);
            B.gitems.resize((size_t)TS * (sizeof(vgl_gvcf_item) / sizeof(int32_t)));
            B.fdp.resize(N); B.ldp.resize(N); B.fpl.resize((size_t)G * N); B.lpl.resize((size_t)G * N);
            B.contig.resize(TS); B.pos0.resize(TS);
            memset(&B.g, 0, sizeof B.g);
            B.g.items = (vgl_gvcf_item*)B.gitems.data(); B.g.text = B.text.data(); B.g.text_cap = B.text_cap;
            B.g.record_offsets = B.toff.data(); B.g.block_offsets = B.boff.data();
            B.g.first_dp = B.fdp.data(); B.g.first_pl = B.fpl.data(); B.g.last_dp = B.ldp.data(); B.g.last_pl = B.lpl.data();
            return;
        }
        if (a.add_gl) { B.gl.resize(E * G); B.o.gl = B.gl.data(); }
        if (a.add_pl) { B.pl.resize(E * G); B.o.pl = B.pl.data(); }
        if (a.add_gp) { B.gp.resize(E * G); B.o.gp = B.gp.data(); }
        if (a.add_fmt_ad) { B.ad.resize(E * A); B.o.fmt_ad = B.ad.data(); }
        if (a.add_fmt_adf) { B.adf.resize(E * A); B.o.fmt_adf = B.adf.data(); }
        if (a.add_fmt_adr) { B.adr.resize(E * A); B.o.fmt_adr = B.adr.data(); }
    };
    if (dstream) {
        // The largest head of a site, from what build_record writes.  Text: chrom, id, qual, filt and the input's own INFO; POS (at most 20
        // digits); REF and ALT (at most five alleles, the longest "<NON_REF>", with commas: 32); eight tabs; and per INFO tag this run adds
        // ";KEY=" (at most 5) and its numbers with commas, 16 bytes each (an int32 takes 11, kputd's forms and %g of a float 13, the binary
        // placeholder "~%08x" 9): DP 1, QS and the AD tags one per allele (A), I16 16.  BCF (encode_head): 8 bytes of lengths, 24 of fixed
        // fields, and every column typed -- a string or vector costs at most 5 bytes over its text, an added number 4 bytes, and the
        // input's INFO at most twice its text (a one-digit number with its comma becomes a 4-byte float): bounded by the same sum with
        // the INFO doubled and 64 bytes more.  The handle refuses a tile whose heads take more.
        size_t longest = 0;
        for (const Rec& r : vcf.recs) longest = std::max(longest, r.chrom.size() + r.id.size() + r.qual.size() + r.filt.size() + 2 * r.info.size());
        const size_t n_added = (a.add_info_dp ? 1 : 0) + (a.add_qs ? A : 0) + (a.add_i16 ? 16 : 0) + (size_t)A * ((a.add_info_ad ? 1 : 0) + (a.add_info_adf ? 1 : 0) + (a.add_info_adr ? 1 : 0));
        const size_t per_site = longest + 20 + 32 + 8 + 6 * 5 + 16 * n_added + 64 + 64;
        const int64_t max_head = (int64_t)TS * (int64_t)per_site;
        for (int d = 0; d < D; d++) {
            const int64_t cap = vgl_ctx_text_bound(ctxs[d], TS);
            if (cap < 0) die("--device-stream 1: %s", vgl_last_error());
            if (vgl_stream_host_create(devices[d], R / D, TS, max_head, std::max<int64_t>(cap, 1), &hstream[d]) != VGL_OK)
                die("--device-stream 1: %s (device %d)", vgl_last_error(), devices[d]);
            if (vgl_ctx_text_device(ctxs[d], 1) != VGL_OK) die("--device-stream 1: %s", vgl_last_error());
        }
    }
    alloc_entry(0);
    // one worker per device: simulates the tiles handed to it, in order
    struct Worker { std::thread th; std::mutex m; std::condition_variable cv; std::vector<TileBufs*> q; size_t head = 0; bool stop = false;
                    long tiles = 0, sites = 0; double t_first = -1.0, t_last = 0.0; double text_bytes = 0.0; };          // --verbose 1: what this device did (written by its own thread, read after the join)
    // bytes a finished tile brings back over the link, per site (the FORMAT arrays dominate: sample-major slabs, copied whole)
    // (--device-text 1 / --device-gvcf 1 / --device-bcf 1: the text or the encoded vectors instead of the FORMAT arrays, counted as they come back)
    const double bytes_per_site = rec0 ? 64.0 : (double)N * ((want_dp ? 4.0 : 0.0) + (dtext || dgvcf ? 0.0 : 4.0 * G * ((a.add_gl ? 1 : 0) + (a.add_pl ? 1 : 0) + (a.add_gp ? 1 : 0)) +
                                               4.0 * A * ((a.add_fmt_ad ? 1 : 0) + (a.add_fmt_adf ? 1 : 0) + (a.add_fmt_adr ? 1 : 0)))) + 64.0;
    std::vector<std::unique_ptr<Worker>> workers(D);
    for (int d = 0; d < D; d++) {
        workers[d].reset(new Worker());
        Worker* W = workers[d].get();
        vgl_ctx* ctx = ctxs[d];
        const int32_t* dps = a.gvcf_dps.data(); const int32_t n_dps = (int32_t)a.gvcf_dps.size();
        vgl_stream_host* hs = hstream[d];
        W->th = std::thread([W, ctx, hs, &now, dtext, dgvcf, dpile, dps, n_dps]() {
            // a tile is submitted (vgl_simulate_tile_async) before the previous one is waited for: its kernels run while the
            // previous tile's tags are still on their way to the host
            TileBufs* prev = nullptr; int32_t prev_ticket = 0;
            for (;;) {
                TileBufs* B = nullptr;
                {
                    std::unique_lock<std::mutex> lk(W->m);
                    if (!prev) W->cv.wait(lk, [&] { return W->stop || W->head < W->q.size(); });
                    if (W->head < W->q.size()) B = W->q[W->head++];
                    else if (!prev) return;
                }
                int32_t ticket = 0;
                if (B && W->t_first < 0.0) W->t_first = now();
                if (B && dpile && vgl_ctx_pileup_next(ctx, &B->pt) != VGL_OK) die("%s", vgl_last_error());   // (a side channel of the tile call below)
                if (B && !dtext && !dgvcf && vgl_simulate_tile_async(ctx, B->t0, B->ns, B->gt.data(), &B->o, &ticket) != VGL_OK) die("%s", vgl_last_error());
                if (B && dgvcf && vgl_simulate_tile_gvcf_async(ctx, B->t0, B->ns, B->gt.data(), B->contig.data(), B->pos0.data(), dps, n_dps, &B->o, &B->g,
                                                               &ticket) != VGL_OK)
                    die("%s", vgl_last_error());
                // (--device-stream 1: the text stays on the device, in the entry's body buffer of the stream handle)
                if (B && dtext && vgl_simulate_tile_text_async(ctx, B->t0, B->ns, B->gt.data(), &B->o, hs ? vgl_stream_host_body(hs, B->sbuf) : B->text.data(),
                                                               B->text_cap, B->toff.data(), &ticket) != VGL_OK)
                    die("%s", vgl_last_error());
                if (prev) {
                    if (vgl_tile_wait(ctx, prev_ticket) != VGL_OK) die("%s", vgl_last_error());
                    if (dtext && !hs) W->text_bytes += (double)prev->toff[prev->ns];
                    if (dgvcf) W->text_bytes += (double)prev->g.text_needed;
                    if (dpile) W->text_bytes += (double)prev->pt.text_needed;
                    W->tiles += 1; W->sites += prev->ns; W->t_last = now();
                    { std::lock_guard<std::mutex> lk(prev->m); prev->done = true; }
                    prev->cv.notify_all();
                }
                prev = B; prev_ticket = ticket;
            }
        });
    }

    long n_out = 0, n_skipped = 0;
    std::string line, tsv;
    GvcfBlocker gv;
    std::vector<std::string> enc;
    gv.block_dps = a.gvcf_dps;
    // one simulated record of a tile: the eight fixed columns as text, the allele strings and the
    // typed FORMAT arrays (reads the tile buffers only: records of a tile are built on several threads)
    auto build_record = [&](const TileBufs& B, int i, std::string& line, std::vector<std::string>& al, std::vector<vsink::FmtDesc>& fmt) {
        const SiteMeta& S = B.meta[i];
        const int nA = B.na[i], nG = nA * (nA + 1) / 2;
        char hb[64];
        line += S.rec->chrom; snprintf(hb, sizeof hb, "\t%ld\t", S.pos0 + 1); line += hb;
        line += S.rec->id; line += '\t';
        // alleles (vcfgl.cpp:739-762; no-reads site :250-280)
        al.clear();
        for (int k = 0; k < nA; k++) { const int b = B.a2b[(size_t)i * 5 + k]; al.push_back(b == 4 ? nonref : (b >= 0 ? std::string(1, "ACGT"[b]) : ".")); }
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
        if (dtext || dgvcf) return;                              // the sample columns come from the device
        const size_t sN = (size_t)N, sG = (size_t)nG, sA = (size_t)nA;
        if (a.add_fmt_dp) fmt.push_back({"DP", false, 1, &B.dp[(size_t)i * N], 1, sN});
        if (a.add_gl) fmt.push_back({"GL", true, nG, &B.gl[(size_t)i * G * N], sG, 1});
        if (a.add_pl) fmt.push_back({"PL", false, nG, &B.pl[(size_t)i * G * N], sG, 1});
        if (a.add_gp) fmt.push_back({"GP", true, nG, &B.gp[(size_t)i * G * N], sG, 1});
        if (a.add_fmt_ad) fmt.push_back({"AD", false, nA, &B.ad[(size_t)i * A * N], sA, 1});
        if (a.add_fmt_adf) fmt.push_back({"ADF", false, nA, &B.adf[(size_t)i * A * N], sA, 1});
        if (a.add_fmt_adr) fmt.push_back({"ADR", false, nA, &B.adr[(size_t)i * A * N], sA, 1});
    };
    // --device-gvcf 1: a tile's items in order.  Records and blocks get their fixed columns here (in parallel) and their sample
    // columns from the device; the tile's last block stays open on the host (GvcfBlocker's state) and takes in the first block of a
    // later tile that continues it (same contig, pos0 <= END + 1, same range): min / lexicographic-min aggregates, founder from the left
    auto site_alleles = [&](const TileBufs& B, int i) {
        std::string s;
        for (int k = 0; k < B.na[i]; k++) { const int b = B.a2b[(size_t)i * 5 + k]; if (k) s += ','; s += b == 4 ? std::string(nonref) : (b >= 0 ? std::string(1, "ACGT"[b]) : std::string(".")); }
        return s.empty() ? std::string(".") : s;
    };
    auto pl_count_die = [&](int nA) { die("Unexpected number of PL values: %d", N * nA * (nA + 1) / 2); };
    auto write_gvcf_tile = [&](TileBufs& B) {
        const vgl_gvcf_tile& g = B.g;
        const int ni = g.n_items;
        const vgl_gvcf_item* it = g.items;
        bool merge = false;
        if (ni > 0 && it[0].kind == VGL_GVCF_BLOCK && gv.current_dpr != 0) {
            const int f = it[0].first;
            merge = B.meta[f].rec->chrom == gv.chrom && B.meta[f].pos0 <= gv.end_pos + 1 && it[0].dpr == gv.current_dpr;
            if (merge && (B.na[f] != 2 || gv.pl.size() != (size_t)N * 3)) pl_count_die(B.na[f]);
        }
        if (g.error_site >= 0) pl_count_die(B.na[g.error_site]);
        enc.resize(std::max(ni, 1));
        vsink::parallel_for(ni, enc_threads, [&](int k) {
            enc[k].clear();
            const vgl_gvcf_item& t = it[k];
            std::string sh8; std::string& col = dbcf ? sh8 : enc[k];    // --device-bcf 1: the fixed columns become the record's shared block
            if (t.kind == VGL_GVCF_RECORD) {
                std::vector<std::string> al; std::vector<vsink::FmtDesc> fmt; build_record(B, t.first, col, al, fmt);
                if (dbcf) out.encode_head(sh8, (uint32_t)n_fmt, (size_t)(B.toff[t.first + 1] - B.toff[t.first]), enc[k]);
                return;
            }
            if ((k == 0 && merge) || k == ni - 1) return;            // carried on the host
            const int f = t.founder;
            GvcfBlocker::fixed_columns(col, out, B.meta[f].rec->chrom, B.meta[f].pos0, B.meta[t.last].pos0, site_alleles(B, f), t.min_dp,
                                       a.add_qs ? &B.qs[(size_t)f * A] : nullptr, a.add_qs ? (size_t)B.na[f] : 0);
            if (dbcf) out.encode_head(sh8, 2, (size_t)(B.boff[t.block + 1] - B.boff[t.block]), enc[k]);        // PL, DP
        });
        lap(4);
        for (int k = 0; k < ni; k++) {
            const vgl_gvcf_item& t = it[k];
            if (t.kind == VGL_GVCF_BLOCK && k == 0 && merge) {
                if (gv.min_dp > t.min_dp) gv.min_dp = t.min_dp;
                for (int s = 0; s < N; ++s) {
                    if (gv.dp[s] > B.fdp[s]) gv.dp[s] = B.fdp[s];
                    const int32_t p1 = B.fpl[(size_t)3 * s + 1], p2 = B.fpl[(size_t)3 * s + 2];
                    if (gv.pl[3 * s + 1] > p1) { gv.pl[3 * s + 1] = p1; gv.pl[3 * s + 2] = p2; }
                    else if (gv.pl[3 * s + 1] == p1 && gv.pl[3 * s + 2] > p2) gv.pl[3 * s + 2] = p2;
                }
                gv.end_pos = B.meta[t.last].pos0;
                if (k < ni - 1) { gv.emit(out, N); n_out++; }
                continue;
            }
            if (gv.current_dpr != 0) { gv.emit(out, N); n_out++; }
            if (t.kind == VGL_GVCF_BLOCK && k == ni - 1) {               // the tile's last block: open until a later tile decides
                const int f = t.founder, nA = B.na[f], nG = nA * (nA + 1) / 2;
                const int32_t* dp = (ni == 1) ? B.fdp.data() : B.ldp.data();
                const int32_t* pl = (ni == 1) ? B.fpl.data() : B.lpl.data();
                gv.dp.assign(dp, dp + N); gv.pl.assign(pl, pl + (size_t)N * nG);
                gv.qsum.clear(); if (a.add_qs) gv.qsum.assign(&B.qs[(size_t)f * A], &B.qs[(size_t)f * A] + nA);
                gv.chrom = B.meta[f].rec->chrom; gv.start_pos = B.meta[f].pos0; gv.end_pos = B.meta[t.last].pos0;
                gv.alleles = site_alleles(B, f); gv.min_dp = t.min_dp; gv.current_dpr = t.dpr;
                continue;
            }
            out.put(enc[k]);
            if (t.kind == VGL_GVCF_BLOCK) out.put(B.text.data() + B.boff[t.block], (size_t)(B.boff[t.block + 1] - B.boff[t.block]));
            else out.put(B.text.data() + B.toff[t.first], (size_t)(B.toff[t.first + 1] - B.toff[t.first]));
            n_out++;
        }
        lap(5);
    };
    // --device-stream 1: bytes of heads and offsets sent up and of members brought back, per device (--verbose 1)
    std::vector<double> stream_up(D, 0.0), stream_down(D, 0.0);
    // the members of a tile whose heads were submitted: to the file, in tile order
    auto retire_tile = [&](TileBufs& B) {
        const uint8_t* m; int64_t mn, raw;
        if (vgl_stream_host_wait(hstream[B.dev], B.sticket, &m, &mn, &raw) != VGL_OK) die("--device-stream 1: %s", vgl_last_error());
        if (raw != B.hoff[B.ns] + B.toff[B.ns]) die("--device-stream 1: the device assembled %lld bytes of %lld", (long long)raw, (long long)(B.hoff[B.ns] + B.toff[B.ns]));
        out.put_members(m, (size_t)mn);
        stream_down[B.dev] += (double)mn;
        B.sticket = -1;
    };
    // everything the writer does with one finished tile, in site order (TSV lines, pileup, gVCF blocks, records)
    auto write_tile = [&](TileBufs& B) {
        const int ns = B.ns;
        if (rec0) { for (int i = 0; i < ns; i++) if (B.st[i] < 0) n_skipped++; return; }
        for (int i = 0; i < ns; i++) {
            const SiteMeta& S = B.meta[i];
            if ((dump_pick || dump_reads) && B.st[i] != VGL_SITE_SKIP_EMPTY && B.idp[i] > 0) {      // sites that reach the read loop (vcfgl.cpp:396-404)
                tsv.clear();
                char hb[96];
                if (dump_pick) for (int s = 0; s < N; s++) {                                   // vcfgl.cpp:430-435
                    tsv += "base_pick_error_prob\t"; tsv += vcf.samples[s]; tsv += '\t'; tsv += S.rec->chrom;
                    snprintf(hb, sizeof hb, "\t%ld\tNA\t%f\n", S.pos0 + 1, B.pick[i]); tsv += hb;
                }
                if (dump_reads) for (int s = 0; s < N; s++) {                                  // vcfgl.cpp:533-554
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
            if (pile_fp && B.st[i] != VGL_SITE_SKIP_EMPTY) {              // vcfgl.cpp:414-416, 616-634 (printed before skip decisions)
                const double t_pile = now();
                line.clear();
                char hb[64]; snprintf(hb, sizeof hb, "\t%ld\t%c", S.pos0 + 1, S.ref_char);
                line += S.rec->chrom; line += hb;
                if (dpile) {                                                // the prefix here, the sample columns and the newline from the device
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
                const double dt = now() - t_pile;                          // --verbose 1: the pileup's own stage, out of write/compress
                t_stage[8] += dt; t_mark += dt;
            }
            if (B.st[i] < 0) { n_skipped++; continue; }
            if (!a.do_gvcf || dgvcf) continue;                           // plain records, device gVCF: written below
            // gVCF: write_record_values (vcfgl.cpp:167-206) carries the open block from record to record (and from tile to
            // tile, whichever device simulated it)
            const int nA = B.na[i];
            std::vector<std::string> al; std::vector<vsink::FmtDesc> fmt;
            line.clear();
            build_record(B, i, line, al, fmt);
            SiteView sv;
            sv.chrom = &S.rec->chrom; sv.pos0 = S.pos0; sv.n_obs = B.nobs[i]; sv.n_alleles = nA; sv.N = N; sv.G = G;
            sv.dp = &B.dp[(size_t)i * N]; sv.pl = &B.pl[(size_t)i * G * N]; sv.qs = a.add_qs ? &B.qs[(size_t)i * A] : nullptr;
            sv.alleles = al[0]; for (size_t k = 1; k < al.size(); k++) { sv.alleles += ','; sv.alleles += al[k]; }
            int ret = gv.prepare(&sv);
            if (ret == GvcfBlocker::FLUSH_BLOCK) { gv.emit(out, N); n_out++; ret = gv.prepare(&sv); }
            if (ret == GvcfBlocker::WRITE_SIMREC) { out.write_rec(line, fmt); n_out++; }
        }
        if (dgvcf) write_gvcf_tile(B);
        if (!a.do_gvcf) {
            enc.resize(ns);
            vsink::parallel_for(ns, enc_threads, [&](int i) {
                enc[i].clear();
                if (B.st[i] < 0) return;
                std::string sh; std::vector<std::string> al; std::vector<vsink::FmtDesc> fmt;
                build_record(B, i, sh, al, fmt);
                if (dbcf) { out.encode_head(sh, (uint32_t)n_fmt, (size_t)(B.toff[i + 1] - B.toff[i]), enc[i]); return; }
                if (dtext) { enc[i] = std::move(sh); return; }
                out.encode_rec(sh, fmt, enc[i]);
            });
            if (dstream) {                                          // the heads go up; the device puts the records together and compresses them
                B.heads.clear();
                for (int i = 0; i < ns; i++) { B.hoff[i] = (int64_t)B.heads.size(); B.heads += enc[i]; if (B.st[i] >= 0) n_out++; }
                B.hoff[ns] = (int64_t)B.heads.size();
                lap(4);
                if (vgl_stream_host_submit(hstream[B.dev], B.sbuf, ns, (const uint8_t*)B.heads.data(), B.hoff.data(), B.toff.data(), &B.sticket) != VGL_OK)
                    die("--device-stream 1: %s", vgl_last_error());
                stream_up[B.dev] += (double)B.heads.size() + 16.0 * (ns + 1);
                lap(5);
                return;
            }
            lap(4);
            for (int i = 0; i < ns; i++) if (B.st[i] >= 0) {
                out.put(enc[i]);
                if (dtext) out.put(B.text.data() + B.toff[i], (size_t)(B.toff[i + 1] - B.toff[i]));     // tab, FORMAT, the sample columns, newline
                n_out++;
            }
            lap(5);
        }
    };

    // ---- the tile ring: produce (decode sites, hand the tile to its device) up to R tiles ahead, write in order
    size_t produced = 0, consumed = 0;
    size_t retired = 0;                                         // --device-stream 1: tiles whose members are written (one behind `consumed`); else = consumed
    bool eof = false;
    std::map<std::string, int32_t> contig_ids; const std::string* last_chrom = nullptr; int32_t last_id = 0;
    lap(6);
    for (;;) {
        while (!eof && produced - retired < (size_t)R) {
            alloc_entry(produced % R);
            TileBufs& B = *ring[produced % R];
            B.ns = 0; B.t0 = (int64_t)n_sites_total; B.done = false; B.dev = (int)(produced % D);
            while (B.ns < TS && stream.next(&B.gt[(size_t)B.ns * N], B.meta[B.ns])) B.ns++;
            if (B.ns < TS) eof = true;
            if (B.ns == 0) break;
            if (dgvcf) for (int i = 0; i < B.ns; i++) {                 // contig ids: equal for equal names (the device compares ids)
                const std::string& c = B.meta[i].rec->chrom;
                if (last_chrom == nullptr || *last_chrom != c) {
                    auto ins = contig_ids.emplace(c, (int32_t)contig_ids.size());
                    last_id = ins.first->second; last_chrom = &ins.first->first;
                }
                B.contig[i] = last_id; B.pos0[i] = B.meta[i].pos0;
            }
            n_sites_total += (size_t)B.ns;
            PBuf<uint8_t>::device() = devices[B.dev]; PBuf<double>::device() = devices[B.dev];      // dump buffers of this entry: next to its device, like the rest
            if (pile_fp && !dpile) { B.reads.resize((size_t)pile_cap * TS * N); memset(B.reads.data(), 0xFF, (size_t)pile_cap * B.ns * N); B.o.reads = B.reads.data(); B.o.read_capacity = pile_cap; }   // capacity of the per-read dump: the library stages at most read_cap reads; ask generously
            if (want_errp) { B.errp.resize((size_t)pile_cap * TS * N); B.o.read_errp = B.errp.data(); B.o.read_capacity = pile_cap; }
            if (dump_pick) { B.pick.resize(TS); B.o.site_pick_err = B.pick.data(); }
            Worker* W = workers[B.dev].get();
            { std::lock_guard<std::mutex> lk(W->m); W->q.push_back(&B); }
            W->cv.notify_one();
            produced++;
        }
        lap(1);
        if (consumed == produced) break;
        TileBufs& B = *ring[consumed % R];
        { std::unique_lock<std::mutex> lk(B.m); B.cv.wait(lk, [&] { return B.done; }); }
        lap(3);
        write_tile(B);
        lap(5);
        consumed++;
        // --device-stream 1: this tile is being assembled and compressed; meanwhile the one before it is written
        if (dstream) { while (retired + 1 < consumed) { retire_tile(*ring[retired % R]); retired++; } lap(5); }
        else retired = consumed;
    }
    if (dstream) { t_mark = now(); while (retired < consumed) { retire_tile(*ring[retired % R]); retired++; } lap(5); }
    for (auto& W : workers) { { std::lock_guard<std::mutex> lk(W->m); W->stop = true; } W->cv.notify_all(); W->th.join(); }
    if (a.do_gvcf && gv.prepare(nullptr) == GvcfBlocker::FLUSH_BLOCK) { gv.emit(out, N); n_out++; }
    t_mark = now();
    if (!rec0) out.close();
    if (a.print_truth) truth_sink.close();
    if (a.gt_disc) {                                            // every context's table, summed: integer counts, the same for any device count
        const int64_t len = vgl_disc_table_len(N);
        std::vector<int64_t> table((size_t)len, 0), part((size_t)len);
        for (int d = 0; d < D; d++) {
            if (vgl_ctx_discordance_read(ctxs[d], part.data(), 0) != VGL_OK) die("--gt-discordance 1: %s", vgl_last_error());
            for (int64_t k = 0; k < len; k++) table[(size_t)k] += part[(size_t)k];
        }
        const std::string tsv_text = format_discordance(table, vcf.samples, a.disc_gq);
        FILE* fp = fopen((a.out_prefix + ".discordance.tsv").c_str(), "w");
        if (!fp) die("Could not open file: %s.discordance.tsv", a.out_prefix.c_str());
        if (fwrite(tsv_text.data(), 1, tsv_text.size(), fp) != tsv_text.size() || fclose(fp) != 0) die("Could not write file: %s.discordance.tsv", a.out_prefix.c_str());
    }
    lap(5);
    if (pile_fp) { pile.close(); fclose(pile_fp); }
    // contexts and page-locked buffers are not torn down one by one (0.06 s): the process ends below with _exit(), after the run
    // log, and the driver releases everything at once
    lap(7);
    if (a.verbose) {
        // per device: tiles, sites, bytes of tags copied back and the rate over the device's own busy interval (first submit to last
        // completed wait) -- a multi-GPU run shows an idle or slow device (or link) here at once
        for (int d = 0; d < D; d++) {
            const Worker& W = *workers[d];
            vgl_ctx_info_t ci; memset(&ci, 0, sizeof ci); ci.size = (int32_t)sizeof ci;
            (void)vgl_ctx_info(ctxs[d], &ci);
            const double dt = W.t_last - W.t_first, gb = (bytes_per_site * (double)W.sites + W.text_bytes + stream_down[d]) / 1e9;
            if (dstream) fprintf(stderr, "[device %d] --device-stream 1: %.6f GB of heads and offsets sent up, %.6f GB of BGZF members copied back\n", devices[d], stream_up[d] / 1e9, stream_down[d] / 1e9);
            fprintf(stderr, "[device %d] %ld tiles, %ld sites, %.3f GB of tags copied back in %.3f s = %.1f GB/s, %.3g evaluations/s; context: %.2f GB workspace, k_sample build %d, fused %d (split %d)\n",
                    devices[d], W.tiles, W.sites, gb, dt > 0 ? dt : 0.0, dt > 0 ? gb / dt : 0.0, dt > 0 ? (double)W.sites * N / dt : 0.0,
                    (double)ci.workspace_bytes / 1e9, ci.sample_lean, ci.fused, ci.fused_split);
        }
    }
    if (a.verbose) fprintf(stderr, "\n[timing] read input %.3f s, decode sites %.3f s, device context(s) %.3f s, waiting for the device(s) (simulation incl. PCIe, overlapped with the writer) %.3f s, encode %.3f s, write/compress %.3f s, tile buffers %.3f s, teardown %.3f s, pileup %.3f s\n",
                           t_stage[0], t_stage[1], t_stage[2], t_stage[3], t_stage[4], t_stage[5], t_stage[6], t_stage[7], t_stage[8]);
    // the parts of "read input" (the HIP runtime's start-up, which the reading overlaps with, is what remains of it)
    if (a.verbose) fprintf(stderr, "[input] --device-input %d: %ld lines parsed on the device, %ld of them again on the host, %.3f GB of text sent up; file read %.3f s, line scan %.3f s, fixed columns %.3f s, device parse and wait %.3f s, host %s %.3f s\n",
                           a.device_input, in_stats.lines_dev, a.device_input ? in_stats.lines_host : 0L, in_stats.text_up / 1e9, in_stats.t_read, in_stats.t_scan, in_stats.t_fixed,
                           in_stats.t_dev, a.device_input ? "re-parse" : "parse", in_stats.t_host);
    if (a.verbose) {
        if (!a.device_inflate) fprintf(stderr, "[input] --device-inflate 0: the host read the file (zlib)\n");
        else fprintf(stderr, "[input] --device-inflate 1: %ld members inflated on the device, %lld compressed bytes sent up, %lld inflated bytes received, %s%s; inflate stage %.3f s of file read %.3f s\n",
                     in_stats.members_dev, (long long)in_stats.inflate_up, (long long)in_stats.inflate_down, in_stats.fallback ? "the host read the file (zlib): " : "no fallback",
                     in_stats.fallback ? in_stats.fallback : "", in_stats.t_inflate, in_stats.t_read);
    }
    char sb[512];
    snprintf(sb, sizeof sb, "\n\n-> Simulation finished successfully.\n\nSummary:\n\tNumber of samples: %d\n\tTotal number of sites simulated: %zu\n"
                            "\tNumber of sites included in simulation output file: %ld\n\tNumber of sites skipped: %ld\n", N, n_sites_total, n_out, n_skipped);
    fputs(sb, stderr);
    std::vector<std::string> files;
    if (!rec0) files.push_back("-> Simulation output file: " + a.out_prefix + ext);
    if (a.gt_disc) files.push_back("-> Genotype discordance file: " + a.out_prefix + ".discordance.tsv");
    if (a.print_pileup) files.push_back("-> Pileup output file: " + a.out_prefix + ".pileup.gz");
    if (a.print_truth) files.push_back("-> True genotypes output file: " + a.out_prefix + ".truth" + ext);
    if (a.print_bpe) files.push_back("-> Base pick error output: stdout");
    if (a.print_qs_err) files.push_back("-> QS error output: stdout");
    if (a.print_gl_err) files.push_back("-> GL error output: stdout");
    if (a.print_qscores) files.push_back("-> Qscores output: stdout");
    fflush(stdout);
    runlog.finish(sb, files);
    // a flush that fails here (ENOSPC, EPIPE on stdout's TSV listings) is a failed run; VCFGL_HIP_NORMAL_EXIT=1 leaves through
    // exit() instead of _exit(), so that atexit handlers (profilers, sanitizers) run -- at the price of the piecewise teardown
    const int flush_rc = fflush(NULL);
    if (flush_rc != 0) { fprintf(stderr, "\n[ERROR] could not flush the output streams: %s\n", strerror(errno)); _exit(1); }
    if (getenv("VCFGL_HIP_NORMAL_EXIT")) exit(0);
    _exit(0);
}
