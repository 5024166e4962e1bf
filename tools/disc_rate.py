#!/usr/bin/env python3
"""End-to-end rate of the host program with the discordance tally (--gt-discordance 1), with and without records, on a synthetic
input of SITES x SAMPLES phased binary genotypes (tools/cli_rate.py's input and flags).  Everything is inside the measured wall
time: process start, input parsing, simulation, and -- where records are written -- encoding, assembly, compression and the file.
The settings alternate, DISC_REPS times each (default 3), and are reported as min / median / max:
    parent      DISC_PARENT_BIN=path: another build of the program (one that does not know the flags) writing the records
    records     -O b --device-bcf 1 --device-stream 1 --device-bgzf 1, --gt-discordance 0
    records+gt  the same with --gt-discordance 1
    table only  --records 0 --gt-discordance 1
The two tables must be the same file; the two record files the same stream but for their ##source= lines.
usage (GPU box): python tools/disc_rate.py [sites] [samples]"""
import gzip, hashlib, os, struct, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
d = tempfile.mkdtemp(prefix="discrate")
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
flags = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2".split() + os.environ.get("DISC_EXTRA", "").split()
rec = ["-O", "b", "--device-bcf", "1", "--device-stream", "1", "--device-bgzf", "1"]


def bcf_digest(fn):
    """sha1 of a BCF stream without the ##source= lines of its header"""
    raw = gzip.decompress(open(fn, "rb").read())
    l_text = struct.unpack_from("<I", raw, 5)[0]
    h = hashlib.sha1(b"\n".join(l for l in raw[9:9 + l_text].split(b"\n") if not l.startswith(b"##source=")))
    h.update(memoryview(raw)[9 + l_text:])
    return h.hexdigest()


parent = os.environ.get("DISC_PARENT_BIN")
settings = ([("parent", parent, rec)] if parent else []) + [
    ("records", BIN, rec + ["--gt-discordance", "0"]), ("records+gt", BIN, rec + ["--gt-discordance", "1", "--discordance-gq", "6"]),
    ("table only", BIN, ["--records", "0", "--gt-discordance", "1", "--discordance-gq", "6"])]
times, digests, tables = {k: [] for k, _, _ in settings}, {}, {}
for rep in range(int(os.environ.get("DISC_REPS", "3"))):
    for k, (name, prog, extra) in enumerate(settings):
        out = os.path.join(d, f"o{k}")
        t0 = time.perf_counter()
        r = subprocess.run([prog, "-i", vcf, "-o", out, "--verbose", "1"] + flags + extra, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-800:]
        times[name].append(dt)
        size = os.path.getsize(out + ".bcf") / 1e6 if os.path.exists(out + ".bcf") else 0.0
        print(f"{name:11s} run {rep}: {dt:7.2f} s  {S * N / dt:10.3e} evals/s  records {size:8.1f} MB", flush=True)
        if rep == 0:
            for l in r.stderr.splitlines():
                if l.startswith("[timing]") or l.startswith("[device"):
                    print("    " + l, flush=True)
            if size:
                digests[name] = bcf_digest(out + ".bcf")
            if os.path.exists(out + ".discordance.tsv"):
                tables[name] = hashlib.sha1(open(out + ".discordance.tsv", "rb").read()).hexdigest()
        for e in (".bcf", ".discordance.tsv"):
            if os.path.exists(out + e):
                os.remove(out + e)
assert len(set(digests.values())) == 1, "the settings wrote different record streams"
assert len(tables) == 2 and len(set(tables.values())) == 1, "the run with records and the run without wrote different tables"
for name, ts in times.items():
    print(f"  {name:11s} min {min(ts):.2f} s  median {sorted(ts)[len(ts) // 2]:.2f} s  max {max(ts):.2f} s  {S * N / sorted(ts)[len(ts) // 2]:.3e} evals/s at the median", flush=True)
