// cli_args.h -- the flag surface of vcfgl_hip: Args, the usage text, the parser and its range checks
#pragma once
#include "host_util.h"

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
    int records = 1;                   // --records 0: no record file; only the discordance table and / or the fetched GLs come back
    bool fetch = false, fetch_value_given = false;   // --fetch-gl XY: one genotype's GL per site and sample, <prefix>.fetchgl.csv (misc/fetchGl)
    std::string fetch_gl; int fetch_a = -1, fetch_b = -1;      // the two alleles as 0 .. 4 (A, C, G, T, <*>)
    int fetch_value = 0, fetch_mode = VGL_FETCHGL_FLOAT;       // --fetch-gl-value 0|1|2 and the VGL_FETCHGL_* mode it selects
    std::string set_alleles_fn;        // --set-alleles FILE: every record gets the REF/ALT list of its line (misc/setAlleles), relabelled on the device
    int device_inflate = 0;            // --device-inflate 1: a BGZF input is inflated on the first device of the run
    int device_input = 0;              // --device-input 1: the sample columns of the input VCF text parsed on the first device of the run
    int device_bcf_input = 0;          // --device-bcf-input 1: the GT vectors of the input BCF's records decoded on the first device of the run
    int device_inf = 0;                // --device-inf 1: the records of --depth inf made on the device(s), through the tile ring and every --device-* path
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
    "                   discordance table (--gt-discordance 1) and / or the fetched GLs (--fetch-gl XY) come back.  Needs one of the two;\n"
    "                   refused with -printPileup 1, -printTruth 1, -doGVCF 1 and the per-read listings]\n"
    "                   --fetch-gl XY [off; X, Y of A, C, G, T, < (the unobserved allele <*> / <NON_REF>): what misc/fetchGl -gt XY prints for the\n"
    "                   run's record file is written to <prefix>.fetchgl.csv -- per record that has both alleles, POS and the GL of genotype XY\n"
    "                   of every sample (%f, MISSING for a sample without reads), formatted on the device that simulated the tile.  Works with\n"
    "                   every output mode, --device-* path, --devices, --rng-mode, --gt-discordance and --records 0; refused with --depth inf,\n"
    "                   -doGVCF 1 and -addGL 0]\n"
    "                   --fetch-gl-value 0|1|2 [0: the value the tool would read from the file this run writes -- -O v / -O z: the 6 digits of\n"
    "                   the VCF text read back as a float, -O u / -O b: the simulated float; 1: the former; 2: the latter.  Needs --fetch-gl]\n"
    "                   --set-alleles FILE [off; what misc/setAlleles -a FILE does to the run's record file, done on the device before any record\n"
    "                   is written: line i of FILE (REF<TAB>ALT[,ALT...], 1 to 4 ALTs of A, C, G, T and the run's unobserved allele) is the allele\n"
    "                   list of the i-th record; QS, GL, PL and GP are re-indexed to it and renormalised.  Every allele of a line must be one of\n"
    "                   its record's (else the run stops, naming the site).  Works with every output mode, --device-text / -bcf / -stream / -bgzf,\n"
    "                   --devices, --rng-mode, -printTruth and -printPileup (unchanged files); refused with --depth inf, -doGVCF 1,\n"
    "                   --rm-empty-sites 1, --rm-invar-sites with 4, the AD / ADF / ADR tags, --gt-discordance 1, --fetch-gl and --records 0]\n"
    "                   --device-input 0|1 [0: the genotype columns of the input VCF are parsed on the host; 1: on the first GPU of --device /\n"
    "                   --devices: the host reads the file, finds the lines and parses their first nine columns, the text goes up in batches of\n"
    "                   --tile-sites lines and one packed byte per sample comes back.  A line outside the plain grammar (GT alleles of '.' or\n"
    "                   one or two digits, at most two of them) is parsed by the host as with 0.  Same output either way; VCF text input only\n"
    "                   (BCF input is refused), refused with --depth inf; a run without a GPU fails instead of falling back]\n"
    "                   --device-bcf-input 0|1 [0: the genotypes of a BCF input are decoded on one host thread; 1: on the first GPU of --device /\n"
    "                   --devices: the host reads the header, walks the records, decodes their shared blocks on the --encode-threads threads\n"
    "                   and finds each record's GT values, only those bytes go up in batches of --tile-sites records and one packed byte per\n"
    "                   sample comes back.  A record with a missing-value sentinel, a negative value or an allele index beyond its alleles is\n"
    "                   decoded by the host as with 0, and a damaged file is read by the host as with 0.  Same output either way (-printTruth 1\n"
    "                   builds its GT text on the host as before); BCF input only, raw or BGZF (works with --device-inflate 1), refused with\n"
    "                   --depth inf; a run without a GPU fails instead of falling back]\n"
    "                   --device-inflate 0|1 [0: the input is read and inflated by zlib on one host thread; 1: a BGZF input (bgzip'd VCF text, compressed\n"
    "                   BCF) is read as it lies in the file and its members are inflated on the first GPU of --device / --devices, 512 members\n"
    "                   a batch.  A file that is not BGZF (plain text, gzip) and a file with a member the device does not take to its exact end\n"
    "                   are read by zlib as with 0: same bytes either way.  Refused with --depth inf; a run without a GPU fails instead of\n"
    "                   falling back]\n"
    "                   --device-inf 0|1 [0: the records of --depth inf are written by one host thread, value by value, and no device is used; 1: they are\n"
    "                   made on the device(s) -- per tile the allele list of every site and GL 0 / GP 1 / PL 0 at each sample's true genotype,\n"
    "                   -inf / 0 / 255 elsewhere -- and go through the tile ring like simulated records.  Same records either way.  Needs --depth inf\n"
    "                   and one of -addGL / -addGP / -addPL 1.  With it --device-text, --device-bcf, --device-stream, --device-input,\n"
    "                   --device-bcf-input, --device-inflate, --devices, --tile-sites and --encode-threads work as for a finite depth (without it\n"
    "                   --depth inf refuses them); the flags --depth inf ignores on the host (--gl-model, --error-qs, --adjust-qs, --rm-empty-sites,\n"
    "                   --rng-mode, the DP / AD tags ...) are ignored here too.  Refused with -printPileup 1; --gt-discordance 1, --fetch-gl,\n"
    "                   --set-alleles, --records 0, -doGVCF 1, --device-gvcf 1 and --device-pileup 1 stay refused with --depth inf; a run without a\n"
    "                   GPU fails instead of falling back]\n"
    "                   -v --version    -vv    -h --help\n\n";

// the record files' extension: <prefix>.vcf, .vcf.gz or .bcf (the truth file: <prefix>.truth.*)
static const char* output_ext(const Args& a) { const char m = a.output_mode[0]; return m == 'v' ? ".vcf" : m == 'z' ? ".vcf.gz" : ".bcf"; }

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
        else if (f == "--fetch-gl") { a.fetch = true; a.fetch_gl = v; }
        else if (f == "--fetch-gl-value") { a.fetch_value_given = true; a.fetch_value = I(v); }
        else if (f == "--set-alleles") a.set_alleles_fn = v;
        else if (f == "--device-input") a.device_input = I(v);
        else if (f == "--device-inflate") a.device_inflate = I(v);
        else if (f == "--device-bcf-input") a.device_bcf_input = I(v);
        else if (f == "--device-inf") a.device_inf = I(v);
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
    // one genotype's GLs (checked before any GPU work: nothing is written)
    if (a.fetch) {
        static const char letters[] = "ACGT<";
        const char* x = a.fetch_gl.size() == 2 ? strchr(letters, a.fetch_gl[0]) : nullptr;
        const char* y = a.fetch_gl.size() == 2 ? strchr(letters, a.fetch_gl[1]) : nullptr;
        if (!x || !y || !*x || !*y) die("[Bad argument value: '--fetch-gl %s'] A genotype is two of A, C, G, T, < (the unobserved allele).", a.fetch_gl.c_str());
        a.fetch_a = (int)(x - letters); a.fetch_b = (int)(y - letters);
        range(a.fetch_value, 0, 2, "--fetch-gl-value");
        if (a.depth_inf) die("--fetch-gl %s is not supported with --depth inf (no tile is simulated).", a.fetch_gl.c_str());
        if (a.do_gvcf) die("--fetch-gl %s is not supported with -doGVCF 1 (block records).", a.fetch_gl.c_str());
        if (!a.add_gl) die("--fetch-gl %s with -addGL 0: Could not read GL tag.", a.fetch_gl.c_str());
        const bool text_file = a.output_mode == "v" || a.output_mode == "z";
        a.fetch_mode = a.fetch_value == 1 || (a.fetch_value == 0 && text_file) ? VGL_FETCHGL_TEXT : VGL_FETCHGL_FLOAT;
    } else if (a.fetch_value_given) die("--fetch-gl-value %d selects the values of --fetch-gl XY's file: add --fetch-gl XY.", a.fetch_value);
    // a prescribed allele list per record (checked before any GPU work: nothing is written)
    if (!a.set_alleles_fn.empty()) {
        const char* fn = a.set_alleles_fn.c_str();
        if (a.depth_inf) die("--set-alleles %s is not supported with --depth inf (no tile is simulated: the records carry no likelihoods to relabel).", fn);
        if (a.do_gvcf) die("--set-alleles %s is not supported with -doGVCF 1 (a block record stands for many sites).", fn);
        if (a.rm_empty) die("--set-alleles %s is not supported with --rm-empty-sites 1 (the device decides which sites become records: the record index of a line is not known ahead).", fn);
        if (a.rm_invar & 4) die("--set-alleles %s is not supported with --rm-invar-sites %d (bit 4: the device decides which sites become records: the record index of a line is not known ahead).", fn, a.rm_invar);
        if (a.add_fmt_ad || a.add_info_ad || a.add_fmt_adf || a.add_info_adf || a.add_fmt_adr || a.add_info_adr)
            die("--set-alleles %s is not supported with the AD / ADF / ADR tags (misc/setAlleles leaves them with the old allele count: a malformed record).", fn);
        if (a.gt_disc) die("--set-alleles %s is not supported with --gt-discordance 1 (composing the two is not implemented).", fn);
        if (a.fetch) die("--set-alleles %s is not supported with --fetch-gl %s (composing the two is not implemented).", fn, a.fetch_gl.c_str());
        if (!a.records) die("--set-alleles %s is not supported with --records 0 (it changes the record file, and none is written).", fn);
    }
    if (!a.records) {
        if (!a.gt_disc && !a.fetch) die("--records 0 writes no record file: it needs --gt-discordance 1 or --fetch-gl XY, whose file is then the run's only output.");
        if (a.print_pileup) die("--records 0 is not supported with -printPileup 1 (the pileup is a listing of every read).");
        if (a.print_truth) die("--records 0 is not supported with -printTruth 1 (the truth file is a record file).");
        if (a.do_gvcf) die("--records 0 is not supported with -doGVCF 1 (gVCF blocks are records).");
        if (a.print_bpe || a.print_qs_err || a.print_gl_err || a.print_qscores)
            die("--records 0 is not supported with -printBasePickError / -printQsError / -printGlError / -printQScores 1 (per-read listings).");
        a.device_text = a.device_bcf = a.device_gvcf = a.device_stream = a.device_pileup = 0;      // nothing to format, encode or assemble
    }
    // the records of --depth inf from the device (checked before any GPU work: nothing is written).  --gt-discordance 1, --fetch-gl,
    // --set-alleles and with them --records 0 are refused with --depth inf above; -doGVCF 1 and --device-gvcf 1 below, flag or no flag
    range(a.device_inf, 0, 1, "--device-inf");
    if (a.device_inf) {
        if (!a.depth_inf) die("--device-inf 1 makes the records of --depth inf on the device: it needs --depth inf (a finite --depth / --depths-file is simulated on the device anyway).");
        if (!a.add_gl && !a.add_gp && !a.add_pl) die("--device-inf 1 needs at least one of -addGL 1, -addGP 1 and -addPL 1 (with none of them a record has no sample column to make).");
        if (a.print_pileup) die("--device-inf 1 is not supported with -printPileup 1 (no read is drawn with --depth inf: there is no pileup).");
    }
    const bool host_inf = a.depth_inf && !a.device_inf;         // --depth inf on the host: no device is used, no tile is made
    range(a.device_input, 0, 1, "--device-input");
    if (a.device_input == 1 && host_inf) die("--device-input 1 is not supported with --depth inf (no device is used).");
    range(a.device_bcf_input, 0, 1, "--device-bcf-input");
    if (a.device_bcf_input == 1 && host_inf) die("--device-bcf-input 1 is not supported with --depth inf (no device is used).");
    range(a.device_inflate, 0, 1, "--device-inflate");
    if (a.device_inflate == 1 && host_inf) die("--device-inflate 1 is not supported with --depth inf (no device is used).");
    if (a.device_stream == 1 && host_inf) die("--device-stream 1 is not supported with --depth inf (no tile is simulated).");
    if (a.device_gvcf == 1 && a.depth_inf) die("--device-gvcf 1 is not supported with --depth inf (no tile is simulated).");
    if (a.device_bcf == 1 && host_inf) die("--device-bcf 1 is not supported with --depth inf (no tile is simulated).");
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
        if (host_inf) die("--device-text 1 is not supported with --depth inf (no tile is simulated).");
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
