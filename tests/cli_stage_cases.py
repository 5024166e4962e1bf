"""Random configurations of vcfgl_hip for the differential test of its device stages (tests/test_gpu_cli_stages_fuzz.py), their host
twins, and the comparer of everything two runs wrote.  Importable without a GPU: tests/test_cli_stage_cases_cpu.py holds the generator's
coverage, its determinism, the comparer and the share of configurations the CPU oracle refuses.

draw(rng, tmp_dir) -> Case, one configuration:

  input        random_vcf / random_vcf_gvcf of tests/test_gpu_cli_fuzz.py with the sample count of SAMPLE_COUNTS and 1 to 40 records
               (at most 168 sites after -explode 1), written as plain VCF, bgzip'd VCF, raw BCF or BGZF BCF (CONTAINERS), one in four
               each; BGZF members of 700 or 65280 input bytes, so that a file has one member or many
  reference    random_flags of the same module; then
               kind: 0.22 gVCF (random_vcf_gvcf; -doGVCF 1 --gvcf-dps of 1 to 3 thresholds, and the flags -doGVCF 1 needs),
                     0.14 --depth inf (no missing genotype; the tags --depth inf refuses off; one of GL / GP / PL on), else plain;
               -printTruth 1 with 0.3, -printPileup 1 with 0.3 (never with --depth inf)
  side files   plain runs only: --set-alleles with 0.15 (-doUnobserved 4, the flags it refuses off, a TSV of REF + 1 to 4 ALTs of
               A C G T <*> per record); else --fetch-gl XY --fetch-gl-value 0|1|2 with 0.4 (where -addGL 1) and
               --gt-discordance 1 --discordance-gq 0|3|4|5|6 with 0.35; gVCF runs: the tally with 0.35.  They define output and stay
               in the host twin
  stages       every row of STAGES whose rule admits the configuration, each with 0.6; then rows whose rule needs another row
               that was not drawn are dropped (--device-stream without --device-bcf ...).  --records 0 with 0.5 where it works
  shape        --tile-sites of 1, 3, 7, 4096; --devices of 0 / 0,0 / 0,0,0 (--rng-mode 1 runs on --devices 0); --encode-threads and
               (-O u / -O b only: text output refuses more) --threads of 1, 4

host_twin(case): every row of STAGES at 0, --records 1, --devices 0, --tile-sites 4096, one thread; the side-file requests stay."""
import dataclasses
import gzip
import os
import struct

import numpy as np

import bcf_reader
import bcfin_cases as bc
import inflate_corpus as ic
from test_gpu_cli_fuzz import random_flags, random_vcf, random_vcf_gvcf
from vcfgl_amd import VcfglArgError, VcfglArgs
from vcfgl_amd.recordloop import iter_sites
from vcfgl_amd.vcfio import read_vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
SAMPLE_COUNTS = (1, 2, 5, 63, 64, 65, 130, 257)
CONTAINERS = ("vcf", "vcf.gz", "bcf", "bgzf.bcf")
MODES = ("v", "z", "u", "b")
EXT = {"v": ".vcf", "z": ".vcf.gz", "u": ".bcf", "b": ".bcf"}
TILE_SITES = (1, 3, 7, 4096)
DEVICES = ("0", "0,0", "0,0,0")
NAMES = ("A", "C", "G", "T", "<*>")
CHUNKS, CASES_PER_CHUNK, SEED = 16, 6, 18000          # the fixed seeds of the GPU test: SEED + chunk


def _host_inf(f):
    return "inf" in f and "--device-inf" not in f


# The extension-flag table of README.md / `vcfgl_hip -h` as data: flag -> does the flag at 1 work with these facts?  Facts: "O:<mode>",
# "gvcf", "inf", "pileup", "truth", "in:text" / "in:bcf" (the input's format), "in:bgzf" (its container), "GL" / "GP" / "PL", "disc",
# "fetch", "setal", and the flags of this table that are at 1.
STAGES = {
    "--device-inf": lambda f: "inf" in f and bool(f & {"GL", "GP", "PL"}) and "pileup" not in f,
    "--device-gvcf": lambda f: "gvcf" in f and (bool(f & {"O:v", "O:z"}) or "--device-bcf" in f),
    "--device-text": lambda f: bool(f & {"O:v", "O:z"}) and "gvcf" not in f and not _host_inf(f),
    "--device-bcf": lambda f: bool(f & {"O:u", "O:b"}) and ("gvcf" not in f or "--device-gvcf" in f) and not _host_inf(f),
    "--device-stream": lambda f: "gvcf" not in f and not _host_inf(f) and (("O:b" in f and "--device-bcf" in f) or ("O:z" in f and "--device-text" in f)),
    "--device-pileup": lambda f: "pileup" in f and "inf" not in f,
    "--device-bgzf": lambda f: True,
    "--device-input": lambda f: "in:text" in f and not _host_inf(f),
    "--device-bcf-input": lambda f: "in:bcf" in f and not _host_inf(f),
    "--device-inflate": lambda f: "in:bgzf" in f and not _host_inf(f),
}
# the requests that define output (they stay in the host twin) and --records 0
SIDE = {
    "--set-alleles": lambda f: not f & {"rm_empty", "rm_invar4", "AD", "disc", "fetch", "gvcf", "inf"},
    "--fetch-gl": lambda f: "GL" in f and not f & {"gvcf", "inf", "setal"},
    "--gt-discordance": lambda f: not f & {"inf", "setal"},
    "--records": lambda f: bool(f & {"disc", "fetch"}) and not f & {"truth", "pileup", "gvcf", "setal", "inf"},      # (--records 0)
}
P_STAGE = 0.6


@dataclasses.dataclass
class Case:
    input: str                 # the file the program reads
    vcf: str                   # the same records as plain VCF text (for the CPU oracle)
    container: str
    binary: bool
    n_samples: int
    n_records: int
    n_sites: int
    mode: str                  # -O
    kind: str                  # "plain", "gvcf", "inf"
    ref_flags: list            # the reference's own flags
    side_flags: list           # --set-alleles / --fetch-gl / --gt-discordance: in both runs
    stage_flags: list          # STAGES rows at 1 and --records 0
    shape_flags: list

    def stages(self):
        return tuple(self.stage_flags[i] for i in range(0, len(self.stage_flags), 2) if self.stage_flags[i] != "--records")

    @property
    def records0(self):
        return "--records" in self.stage_flags

    def has(self, flag, value="1"):
        for fl in (self.ref_flags, self.side_flags):
            if flag in fl:
                return value is None or fl[fl.index(flag) + 1] == value
        return False

    def argv(self, out, rng_mode):
        shape = list(self.shape_flags)
        if rng_mode == 1:
            shape[shape.index("--devices") + 1] = "0"          # the serial draw order does not shard
        return ([BIN, "-i", self.input, "-o", out, "-O", self.mode, "--rng-mode", str(rng_mode), "--verbose", "1"] + self.ref_flags +
                self.side_flags + self.stage_flags + shape)


def host_twin(case):
    """the same run on the host stages: one device, one tile size for all, records written"""
    return dataclasses.replace(case, stage_flags=[x for f in STAGES for x in (f, "0")] + ["--records", "1"],
                               shape_flags=["--tile-sites", "4096", "--devices", "0", "--encode-threads", "1", "--threads", "1"])


# ---- input containers -----------------------------------------------------------------------------------------------------------
def bcf_of(vcf):
    """the records of a VcfFile (tests' own reader) as raw BCF: GT as phased / unphased int8 pairs, '.' the missing allele"""
    contigs = list(vcf.contigs)
    extra = [b"##contig=<ID=%s,length=%d,IDX=%d>" % (c.encode(), vcf.contigs[c], i) for i, c in enumerate(contigs) if i]
    out = [bc.bcf_header([s.encode() for s in vcf.samples], contig=contigs[0].encode(), length=vcf.contigs[contigs[0]], extra=extra)]
    for r in vcf.records:
        data = bytearray()
        for s in r.samples:
            tok = s["GT"][0]
            a, b = tok.replace("|", "/").split("/")
            data += bytes([bc.gt_value(-1 if a == "." else int(a)), bc.gt_value(-1 if b == "." else int(b), 1 if "|" in tok else 0)])
        rec = bytearray(bc.bcf_record(r.pos0 + 1, [a.encode() for a in r.alleles], len(vcf.samples), [(bc.GT, 1, 2, bytes(data))]))
        struct.pack_into("<i", rec, 8, contigs.index(r.chrom))                      # CHROM (bcf_record writes contig 0)
        out.append(bytes(rec))
    return b"".join(out)


def write_container(rng, vcf_path, container, path):
    data = open(vcf_path, "rb").read()
    if "bcf" in container:
        data = bcf_of(read_vcf(vcf_path))
    if container in ("vcf.gz", "bgzf.bcf"):
        data = ic.bgzf_level6(data, int(rng.choice([700, ic.M])))
    with open(path, "wb") as f:
        f.write(data)


# ---- the reference flags ----------------------------------------------------------------------------------------------------------
def _set(flags, key, value):
    if key in flags:
        flags[flags.index(key) + 1] = str(value)
    else:
        flags += [key, str(value)]


def _get(flags, key, default="0"):
    return flags[flags.index(key) + 1] if key in flags else default


def _drop(flags, key):
    if key in flags:
        i = flags.index(key)
        del flags[i:i + 2]


AD_TAGS = ("-addFormatAD", "-addInfoAD", "-addFormatADF", "-addInfoADF", "-addFormatADR", "-addInfoADR")


def _valid_flags(rng, tmp, N, binary):
    while True:
        flags = random_flags(rng, tmp, N, binary)
        try:
            VcfglArgs.from_argv(flags).validate()
            return flags
        except VcfglArgError:
            continue


def _facts(case_mode, kind, container, ref, side):
    f = {"O:" + case_mode, "in:bcf" if "bcf" in container else "in:text"}
    if container in ("vcf.gz", "bgzf.bcf"):
        f.add("in:bgzf")
    if kind != "plain":
        f.add(kind)
    for key, fact in (("-printPileup", "pileup"), ("-printTruth", "truth"), ("-addGL", "GL"), ("-addGP", "GP"), ("-addPL", "PL"),
                      ("--rm-empty-sites", "rm_empty")):
        if _get(ref, key, "1" if key == "-addGL" else "0") == "1":
            f.add(fact)
    if int(_get(ref, "--rm-invar-sites")) & 4:
        f.add("rm_invar4")
    if any(_get(ref, k) == "1" for k in AD_TAGS):
        f.add("AD")
    for key, fact in (("--gt-discordance", "disc"), ("--fetch-gl", "fetch"), ("--set-alleles", "setal")):
        if key in side:
            f.add(fact)
    return f


def draw(rng, tmp_dir):
    """one configuration; its files are written to tmp_dir (a directory of its own per case: the flag files have fixed names)"""
    tmp_dir = str(tmp_dir)
    os.makedirs(tmp_dir, exist_ok=True)
    N = int(rng.choice(SAMPLE_COUNTS))
    S = int(rng.integers(1, 41))
    binary = bool(rng.integers(0, 2))
    container = CONTAINERS[int(rng.integers(0, 4))]
    mode = MODES[int(rng.integers(0, 4))]
    u = rng.random()
    kind = "gvcf" if u < 0.22 else "inf" if u < 0.36 else "plain"
    vcf = os.path.join(tmp_dir, "in.vcf")
    if kind == "gvcf":
        random_vcf_gvcf(rng, vcf, binary, N=N, S=max(S - 2, 2))           # (it adds two records of a second contig)
    else:
        random_vcf(rng, vcf, binary, N=N, S=S, miss=0.0 if kind == "inf" else None)
    inp = os.path.join(tmp_dir, "in." + container)
    if container != "vcf":
        write_container(rng, vcf, container, inp)
    ref = _valid_flags(rng, tmp_dir, N, binary)
    side = []
    if kind == "gvcf":
        _set(ref, "--rm-invar-sites", 0); _set(ref, "-doUnobserved", int(rng.choice([1, 2, 1, 2, 4, 5])))
        _set(ref, "-addPL", 1); _set(ref, "-addFormatDP", 1)
        dps = sorted(set(int(x) for x in rng.choice([1, 2, 3, 5, 8], size=int(rng.integers(1, 4)))))
        ref += ["-doGVCF", "1", "--gvcf-dps", ",".join(str(d) for d in dps)]
    elif kind == "inf":
        _drop(ref, "--depths-file"); _set(ref, "--depth", "inf")
        _set(ref, "-addQS", 0); _set(ref, "-addI16", 0); _set(ref, "--adjust-qs", 0)
        _set(ref, "--rm-invar-sites", int(_get(ref, "--rm-invar-sites")) & 3)
        if _get(ref, "-addGL") == _get(ref, "-addGP") == _get(ref, "-addPL") == "0":
            _set(ref, ("-addGL", "-addGP", "-addPL")[int(rng.integers(0, 3))], 1)
    if rng.random() < 0.3:
        ref += ["-printTruth", "1"]
    if kind != "inf" and rng.random() < 0.3:
        ref += ["-printPileup", "1"]
    n_sites = None
    if kind == "plain" and rng.random() < 0.15:                         # --set-alleles: made admissible, then one target per record
        _set(ref, "-doUnobserved", 4); _set(ref, "--rm-empty-sites", 0)
        _set(ref, "--rm-invar-sites", int(_get(ref, "--rm-invar-sites")) & 3)
        for k in AD_TAGS:
            _set(ref, k, 0)
        assert SIDE["--set-alleles"](_facts(mode, kind, container, ref, side))
        n_sites = _count_sites(vcf, ref)
        tsv = os.path.join(tmp_dir, "alleles.tsv")
        with open(tsv, "w") as fh:
            for _ in range(n_sites):
                t = [NAMES[i] for i in rng.permutation(5)[:int(rng.integers(2, 6))]]
                fh.write(t[0] + "\t" + ",".join(t[1:]) + "\n")
        side += ["--set-alleles", tsv]
    facts = _facts(mode, kind, container, ref, side)
    if SIDE["--fetch-gl"](facts) and kind == "plain" and rng.random() < 0.4:
        side += ["--fetch-gl", "".join(rng.choice(list("ACGT<"), size=2)), "--fetch-gl-value", str(int(rng.integers(0, 3)))]
    if SIDE["--gt-discordance"](facts) and rng.random() < 0.35:
        side += ["--gt-discordance", "1", "--discordance-gq", str(int(rng.choice([0, 3, 4, 5, 6])))]
    facts = _facts(mode, kind, container, ref, side)
    # the stages: every admissible row with P_STAGE, then to a fixed point of the rules (a row may need another row)
    on = {f for f in STAGES if rng.random() < P_STAGE}
    while True:
        bad = {f for f in on if not STAGES[f](facts | on)}
        if not bad:
            break
        on -= bad
    stage = [x for f in STAGES if f in on for x in (f, "1")]
    if SIDE["--records"](facts) and rng.random() < 0.5:
        stage += ["--records", "0"]
    text_out = mode in "vz"
    shape = ["--tile-sites", str(int(rng.choice(TILE_SITES))), "--devices", DEVICES[int(rng.integers(0, 3))],
             "--encode-threads", str(int(rng.choice([1, 4]))), "--threads", "1" if text_out else str(int(rng.choice([1, 4])))]
    if n_sites is None:
        n_sites = _count_sites(vcf, ref)
    return Case(inp, vcf, container, binary, N, len(read_vcf(vcf).records), n_sites, mode, kind, ref, side, stage, shape)


def _oracle_args(ref):
    """the reference flags the Python mirror of the flag surface knows (--depth inf is outside it: a finite depth stands in)"""
    flags = list(ref)
    if _get(flags, "--depth") == "inf":
        _set(flags, "--depth", "1")
    return VcfglArgs.from_argv(flags).validate()


def _count_sites(vcf, ref):
    return sum(1 for _ in iter_sites(read_vcf(vcf), _oracle_args(ref)))


def fixed_cases(chunk, tmp_dir, seed=SEED, n=CASES_PER_CHUNK):
    """the cases of one chunk of the GPU test"""
    rng = np.random.default_rng(seed + chunk)
    return [draw(rng, os.path.join(str(tmp_dir), "c%d_%d" % (chunk, k))) for k in range(n)]


# ---- what a run wrote, and the comparer ----------------------------------------------------------------------------------------------
def _text_body(path):
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rt") as f:
        return [l for l in f if not l.startswith("##source=")]


def _bcf_stream(path):
    raw = open(path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = b"".join(bcf_reader.bgzf_blocks(raw))
    if raw[:5] != b"BCF\x02\x02":
        return "not a BCF stream", raw
    l_text = struct.unpack_from("<I", raw, 5)[0]
    return [l for l in raw[9:9 + l_text].split(b"\n") if not l.startswith(b"##source=")], raw[9 + l_text:]


def record_file(path):
    """a record or truth file as the single-stage tests read it (test_gpu_cli_vcftext.body, test_gpu_cli_bcf.stream): decompressed,
    ##source= dropped; None where there is no file"""
    if not os.path.exists(path):
        return None
    try:
        return _bcf_stream(path) if path.endswith(".bcf") else _text_body(path)
    except (EOFError, OSError, ValueError, struct.error) as e:                  # a file cut short: a difference, not an exception
        return "unreadable: %s" % e, open(path, "rb").read()


def plain_stderr(stderr):
    """stderr without the [input] / [timing] / [device N] lines of --verbose 1 (the [ERROR] line stays)"""
    return "".join(l for l in stderr.splitlines(True) if not l.startswith("[") or l.startswith("[ERROR]"))


def artifacts(prefix, mode, returncode, stdout, stderr):
    """everything a run wrote; a file that is not there is None"""
    ext = EXT[mode]
    rd = lambda p, op=open: op(p, "rb").read() if os.path.exists(p) else None
    return {"status": returncode, "records": record_file(prefix + ext), "truth": record_file(prefix + ".truth" + ext),
            "pileup": rd(prefix + ".pileup.gz", gzip.open), "discordance": rd(prefix + ".discordance.tsv"),
            "fetchgl": rd(prefix + ".fetchgl.csv"), "stdout": stdout, "stderr": plain_stderr(stderr).replace(prefix, "<prefix>") if returncode != 0 else None}


def differences(a, b, skip=()):
    """the names of the artifacts in which two runs differ.  Of two runs that both exit non-zero only the status and the message are
    compared: the reference flags' refusals (a quality score outside --qs-bins, VGL_E_ADJQ) come from inside a tile, and what a run
    has written by then is decided by --tile-sites and the ring, which the twin does not share."""
    keys = ("status", "stderr") if a["status"] != 0 and b["status"] != 0 else tuple(a)
    return [k for k in keys if k not in skip and a[k] != b[k]]
