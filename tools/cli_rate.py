#!/usr/bin/env python3
"""End-to-end rate of the host program (VCF text in -> GPU simulation -> file out) per output mode and
--threads value, on a synthetic input of SITES x SAMPLES phased binary genotypes.  Everything is
inside the measured wall time: process start, input parsing, PCIe copies, record encoding, compression.
usage (GPU box): python tools/cli_rate.py [sites] [samples]
CLI_BCF_AB=1: every binary mode of the list is run with --device-bcf 0 and --device-bcf 1, alternating, CLI_REPS times each (default 3);
both settings must write the same stream (decompressed, the ##source= lines taken out): checked on every pair.  CLI_PARENT_BIN=path
alternates another build of the program (without the flag) with this one at --device-bcf 0 instead: the run-to-run spread of the two.
CLI_STREAM_AB=1: the modes b and z of the list are run with --device-stream 0 and --device-stream 1 (beside --device-bgzf 1 and the
companion flag: --device-bcf 1 for b, --device-text 1 for z), alternating, CLI_REPS times each; with CLI_PARENT_BIN that build (which
does not know the flag) is the third setting of the rotation.  All settings must write the same decompressed stream."""
import gzip, hashlib, os, struct, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
d = tempfile.mkdtemp(prefix="clirate")
vcf = os.path.join(d, "in.vcf")
gt = synth.binary_sites(0, S, N)                      # packed: low nibble allele 0, high nibble allele 1 (0 = REF, 1 = ALT in ACGT space)
tok = np.array(["0|0", "1|0", "0|1", "1|1"])
with open(vcf, "w") as f:
    f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1))
    f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n")
    for i in range(S):
        g = gt[i]
        idx = (g & 0xF).astype(np.int64) + 2 * (g >> 4).astype(np.int64)
        f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (i + 1) + "\t".join(tok[idx]) + "\n")
print(f"input: {S} sites x {N} samples, {os.path.getsize(vcf) / 1e6:.1f} MB of VCF text")
flags = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2".split() + os.environ.get("CLI_EXTRA", "").split()   # e.g. CLI_EXTRA="--devices 0,0 --tile-sites 8192"
runs = (("v", 0), ("v", 1), ("u", 0), ("u", 1), ("u", 16), ("b", 0), ("b", 1), ("b", 64))
if os.environ.get("CLI_MODES"):                              # e.g. CLI_MODES="u:0,u:16"
    runs = tuple((m.split(":")[0], int(m.split(":")[1])) for m in os.environ["CLI_MODES"].split(","))


def bcf_digest(fn):
    """sha1 of a BCF stream without the ##source= lines of its header"""
    with open(fn, "rb") as f:
        raw = f.read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    l_text = struct.unpack_from("<I", raw, 5)[0]
    h = hashlib.sha1(b"\n".join(l for l in raw[9:9 + l_text].split(b"\n") if not l.startswith(b"##source=")))
    h.update(memoryview(raw)[9 + l_text:])
    return h.hexdigest()


def vcf_digest(fn):
    """sha1 of a bgzip'd VCF stream without its ##source= lines"""
    with gzip.open(fn, "rb") as f:
        raw = f.read()
    return hashlib.sha1(b"\n".join(l for l in raw.split(b"\n") if not l.startswith(b"##source="))).hexdigest()


def ab(mode, threads, stream=False):
    """alternating runs of two (or three) settings of one mode: times, [timing] and [device] lines, output size, equal streams"""
    parent = os.environ.get("CLI_PARENT_BIN")
    ext = ".vcf.gz" if mode == "z" else ".bcf"
    if stream:
        common = ["--device-bgzf", "1"] + (["--device-text", "1"] if mode == "z" else ["--device-bcf", "1"])
        settings = ([("parent", parent, common)] if parent else []) + \
                   [("--device-stream 0", BIN, common + ["--device-stream", "0"]), ("--device-stream 1", BIN, common + ["--device-stream", "1"])]
    else:
        settings = [("parent", parent, []), ("--device-bcf 0", BIN, ["--device-bcf", "0"])] if parent else \
                   [("--device-bcf 0", BIN, ["--device-bcf", "0"]), ("--device-bcf 1", BIN, ["--device-bcf", "1"])]
    th = ["--threads", str(threads)] if threads else []
    times, digests = {k: [] for k, _, _ in settings}, {}
    for rep in range(int(os.environ.get("CLI_REPS", "3"))):
        for k, (name, prog, extra) in enumerate(settings):
            out = os.path.join(d, f"ab_{mode}{threads}_{k}")
            t0 = time.perf_counter()
            r = subprocess.run([prog, "-i", vcf, "-o", out, "-O", mode, "--verbose", "1"] + th + flags + extra, capture_output=True, text=True)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-800:]
            times[name].append(dt)
            print(f"-O {mode} --threads {threads:3d} {name:16s} run {rep}: {dt:7.2f} s  {S * N / dt:10.3e} evals/s  output {os.path.getsize(out + ext) / 1e6:8.1f} MB", flush=True)
            if rep == 0:
                for l in r.stderr.splitlines():
                    if l.startswith("[timing]") or l.startswith("[device"):
                        print("    " + l, flush=True)
                digests[name] = vcf_digest(out + ext) if mode == "z" else bcf_digest(out + ext)
            os.remove(out + ext)
    assert len(set(digests.values())) == 1, f"-O {mode}: the settings wrote different streams"
    for name, ts in times.items():
        print(f"  {name:16s} min {min(ts):.2f} s  median {sorted(ts)[len(ts) // 2]:.2f} s  max {max(ts):.2f} s  spread {(max(ts) - min(ts)) / min(ts) * 100:.1f} %", flush=True)


if os.environ.get("CLI_STREAM_AB"):
    for mode, threads in runs:
        if mode in ("b", "z"):
            ab(mode, threads, stream=True)
    sys.exit(0)
if os.environ.get("CLI_BCF_AB") or os.environ.get("CLI_PARENT_BIN"):
    for mode, threads in runs:
        if mode in ("u", "b"):
            ab(mode, threads)
    sys.exit(0)
for mode, threads in runs:
    out = os.path.join(d, f"o_{mode}{threads}")
    t0 = time.perf_counter()
    th = ["--threads", str(threads)] if threads else []          # 0: not given (the program's default: up to 8 internal threads)
    r = subprocess.run([BIN, "-i", vcf, "-o", out, "-O", mode, "--verbose", "1"] + th + flags, capture_output=True, text=True)
    dt = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-800:]
    fn = out + {"v": ".vcf", "z": ".vcf.gz", "u": ".bcf", "b": ".bcf"}[mode]
    print(f"-O {mode} --threads {threads:3d}: {dt:7.2f} s  {S * N / dt:10.3e} evals/s  output {os.path.getsize(fn) / 1e6:8.1f} MB")
    print("    " + [l for l in r.stderr.splitlines() if l.startswith("[timing]")][-1])
    os.remove(fn)
