#!/usr/bin/env python3
"""End-to-end rate of the host program with --fetch-gl, with and without records, on a synthetic input of SITES x SAMPLES phased
binary genotypes (tools/cli_rate.py's input and flags).  Everything is inside the measured wall time: process start, input parsing,
simulation, and -- where records are written -- formatting, compression and the file.  The settings alternate, FETCH_REPS times each
(default 3), and are reported as min / median / max:
    parent        FETCH_PARENT_BIN=path: another build of the program (one that does not know the flag), -O z --device-text 1 --device-bgzf 1
    records       this build, the same flags
    records+fetch the same with --fetch-gl AC
    fetch only    --records 0 --fetch-gl AC
The two CSVs differ only where the value modes do (-O z: the text's 6 digits; --records 0: the simulated float); the two record files
must be the same stream but for their ##source= lines.  The last run of "fetch only" prints its --verbose 1 stage split.
usage (GPU box): python tools/fetchgl_rate.py [sites] [samples]"""
import gzip, hashlib, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
d = tempfile.mkdtemp(prefix="fetchrate")
vcf = os.path.join(d, "in.vcf")
gt = synth.binary_sites(0, S, N)
tok = np.array(["0|0", "1|0", "0|1", "1|1"])
with open(vcf, "w") as f:
    f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1))
    f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n")
    for i in range(S):
        g = gt[i]
        idx = (g & 0xF).astype(np.int64) + 2 * (g >> 4).astype(np.int64)
        f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (i + 1) + "\t".join(tok[idx]) + "\n")
print(f"input: {S} sites x {N} samples, {os.path.getsize(vcf) / 1e6:.1f} MB of VCF text")
flags = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2".split() + os.environ.get("FETCH_EXTRA", "").split()
rec = ["-O", "z", "--device-text", "1", "--device-bgzf", "1"]


def vcf_digest(fn):
    h = hashlib.sha1()
    for ln in gzip.open(fn, "rb"):
        if not ln.startswith(b"##source="):
            h.update(ln)
    return h.hexdigest()


parent = os.environ.get("FETCH_PARENT_BIN")
settings = ([("parent", parent, rec)] if parent else []) + [
    ("records", BIN, rec), ("records+fetch", BIN, rec + ["--fetch-gl", "AC"]), ("fetch only", BIN, ["--records", "0", "--fetch-gl", "AC"])]
times, digests, last_err = {k: [] for k, _, _ in settings}, {}, {}
for rep in range(int(os.environ.get("FETCH_REPS", "3"))):
    for k, (name, prog, extra) in enumerate(settings):
        out = os.path.join(d, f"o{k}")
        t0 = time.perf_counter()
        r = subprocess.run([prog, "-i", vcf, "-o", out, "--verbose", "1"] + flags + extra, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-800:]
        times[name].append(dt)
        last_err[name] = r.stderr
        csv = os.path.getsize(out + ".fetchgl.csv") / 1e6 if os.path.exists(out + ".fetchgl.csv") else 0.0
        size = os.path.getsize(out + ".vcf.gz") / 1e6 if os.path.exists(out + ".vcf.gz") else 0.0
        print(f"{name:13s} run {rep}: {dt:7.2f} s  {S * N / dt:10.3e} evals/s  records {size:8.1f} MB  csv {csv:8.1f} MB", flush=True)
        if rep == 0 and size:
            digests[name] = vcf_digest(out + ".vcf.gz")
assert len(set(digests.values())) <= 1, digests
print("\n| setting | seconds min / median / max | evaluations/s (median) |\n|---|---|---|")
for name, _, _ in settings:
    t = sorted(times[name])
    print(f"| {name} | {t[0]:.2f} / {t[len(t) // 2]:.2f} / {t[-1]:.2f} | {S * N / t[len(t) // 2]:.1e} |")
print("\nstage split of the last 'fetch only' run:")
print("\n".join(ln for ln in last_err["fetch only"].splitlines() if ln.startswith(("[timing]", "[fetch-gl]", "[device"))))
