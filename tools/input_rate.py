#!/usr/bin/env python3
"""End-to-end time of the host program with the input's genotype columns parsed on the host and on the device (--device-input 0 / 1),
on a synthetic input of SITES x SAMPLES phased binary genotypes (tools/disc_rate.py's input and flags).  Everything is inside the
measured wall time: process start, reading and parsing the input, simulation, and -- where records are written -- encoding,
assembly, compression and the file.  The settings alternate, INPUT_REPS times each (default 3), and are reported as min / median /
max, with the [timing] line of the first run and the [input] line of every run of each:
    parent    INPUT_PARENT_BIN=path: another build of the program (one that does not know the flag)
    input 0   --device-input 0
    input 1   --device-input 1
INPUT_MODE=table (default): --records 0 --gt-discordance 1; INPUT_MODE=records: -O b --device-bcf 1 --device-stream 1 --device-bgzf 1
with the tally.  Every setting must write the same table and, with records, the same decompressed stream but for its ##source= lines.
usage (GPU box): [INPUT_MODE=records] python tools/input_rate.py [sites] [samples]"""
import gzip, hashlib, os, shutil, struct, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
mode = os.environ.get("INPUT_MODE", "table")
d = tempfile.mkdtemp(prefix="inputrate")
vcf = os.path.join(d, "in.vcf")
tok = np.array(["0|0", "1|0", "0|1", "1|1"])
with open(vcf, "w") as f:
    f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1))
    f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n")
    for s0 in range(0, S, 4096):                          # (in blocks: the generator's tables grow with the block)
        gt = synth.binary_sites(s0, min(4096, S - s0), N)
        for i in range(gt.shape[0]):
            g = gt[i]
            idx = (g & 0xF).astype(np.int64) + 2 * (g >> 4).astype(np.int64)
            f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (s0 + i + 1) + "\t".join(tok[idx]) + "\n")
print(f"input: {S} sites x {N} samples, {os.path.getsize(vcf) / 1e6:.1f} MB of VCF text; mode {mode}", flush=True)
flags = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2".split() + os.environ.get("INPUT_EXTRA", "").split()
out_flags = (["-O", "b", "--device-bcf", "1", "--device-stream", "1", "--device-bgzf", "1", "--gt-discordance", "1", "--discordance-gq", "6"]
             if mode == "records" else ["--records", "0", "--gt-discordance", "1", "--discordance-gq", "6"])


def bcf_digest(fn):
    """sha1 of a BCF stream without the ##source= lines of its header"""
    raw = gzip.decompress(open(fn, "rb").read())
    l_text = struct.unpack_from("<I", raw, 5)[0]
    h = hashlib.sha1(b"\n".join(l for l in raw[9:9 + l_text].split(b"\n") if not l.startswith(b"##source=")))
    h.update(memoryview(raw)[9 + l_text:])
    return h.hexdigest()


parent = os.environ.get("INPUT_PARENT_BIN")
settings = ([("parent", parent, [])] if parent else []) + [("input 0", BIN, ["--device-input", "0"]), ("input 1", BIN, ["--device-input", "1"])]
times, digests, tables = {k: [] for k, _, _ in settings}, {}, {}
for rep in range(int(os.environ.get("INPUT_REPS", "3"))):
    for k, (name, prog, extra) in enumerate(settings):
        out = os.path.join(d, f"o{k}")
        t0 = time.perf_counter()
        r = subprocess.run([prog, "-i", vcf, "-o", out, "--verbose", "1"] + flags + out_flags + extra, capture_output=True, text=True, timeout=600)
        dt = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-800:]
        times[name].append(dt)
        print(f"{name:8s} run {rep}: {dt:7.3f} s  {S * N / dt:10.3e} evals/s", flush=True)
        for l in r.stderr.splitlines():                  # the stage split of every run: the start-up of the runtime varies from run to run
            if (l.startswith("[timing]") and rep == 0) or l.startswith("[input]"):
                print("    " + l, flush=True)
        if rep == 0:
            if os.path.exists(out + ".bcf"):
                digests[name] = bcf_digest(out + ".bcf")
            tables[name] = hashlib.sha1(open(out + ".discordance.tsv", "rb").read()).hexdigest()
        for e in (".bcf", ".discordance.tsv"):
            if os.path.exists(out + e):
                os.remove(out + e)
shutil.rmtree(d, ignore_errors=True)
assert len(tables) == len(settings) and len(set(tables.values())) == 1, "the settings wrote different tables"
assert len(set(digests.values())) <= 1 and len(digests) == (len(settings) if mode == "records" else 0), "the settings wrote different record streams"
for name, ts in times.items():
    print(f"  {name:8s} min {min(ts):.3f} s  median {sorted(ts)[len(ts) // 2]:.3f} s  max {max(ts):.3f} s  {S * N / sorted(ts)[len(ts) // 2]:.3e} evals/s at the median", flush=True)

if parent:      # the default path pays nothing: its range must overlap the parent's
    lo, hi = max(min(times["parent"]), min(times["input 0"])), min(max(times["parent"]), max(times["input 0"]))
    print("  --device-input 0 against the parent: " + ("OVERLAP" if lo <= hi else "NO OVERLAP"), flush=True)
    assert lo <= hi, "the --device-input 0 range does not overlap the parent's"
lo, hi = max(min(times["input 0"]), min(times["input 1"])), min(max(times["input 0"]), max(times["input 1"]))
print("  --device-input 1 against 0: " + ("ranges overlap" if lo <= hi else "below" if max(times["input 1"]) < min(times["input 0"]) else "above"), flush=True)
