#!/usr/bin/env python3
"""End-to-end rate of `vcfgl_hip -printPileup 1` with the pileup formatted on the host (--device-pileup 0) and on the device
(--device-pileup 1), on three shapes:
  a  32768 sites x 1000 samples, C3 flags (depth 20, -e 0.01, --error-qs 2, --beta-variance 1e-5, -GL 2), -O b --threads 16 --device-bgzf 1
  b  8192 sites x 1000 samples, the same flags without --device-bgzf (the pileup's BGZF stream is compressed by zlib on one host thread)
  c  the msToGlf-style run --error-qs 0 -e 0.01 -d 1 -GL 2 on 262144 sites x 100 samples, -O b --device-bgzf 1
Everything is inside the wall time (process start, input parsing, PCIe, formatting, compression); the program's own [timing] line follows
(its last field is the pileup's share of the writer thread).  Both settings must write the same .pileup.gz: checked on every pair.
usage (GPU box): python tools/pileup_rate.py [shapes, e.g. abc]
PILEUP_RATE_DIR=dir keeps the inputs there (in_<shape>.vcf); PILEUP_RATE_WRITE_ONLY=1 writes them and prints each shape's flags, e.g. for
a profiler run of one vcfgl_hip process (with VCFGL_HIP_NORMAL_EXIT=1, so that the profiler's exit handlers run)."""
import os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
SHAPES = sys.argv[1] if len(sys.argv) > 1 else "abc"
d = os.environ.get("PILEUP_RATE_DIR") or tempfile.mkdtemp(prefix="pilerate")
os.makedirs(d, exist_ok=True)


def write_vcf(path, S, N):
    gt = synth.binary_sites(0, S, N)
    tok = np.array(["0|0", "1|0", "0|1", "1|1"])
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1))
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n")
        for i in range(S):
            g = gt[i]
            f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (i + 1) + "\t".join(tok[(g & 0xF).astype(np.int64) + 2 * (g >> 4).astype(np.int64)]) + "\n")


C3 = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2 -printPileup 1"
shapes = {
    "a": dict(S=32768, N=1000, flags=C3 + " -O b --threads 16 --device-bgzf 1"),
    "b": dict(S=8192, N=1000, flags=C3 + " -O b --threads 16"),
    "c": dict(S=262144, N=100, flags="--seed 42 --error-qs 0 -e 0.01 -d 1 -GL 2 -printPileup 1 -O b --device-bgzf 1"),
}
for name in SHAPES:
    sh = shapes[name]
    vcf = os.path.join(d, f"in_{name}.vcf")
    if not os.path.exists(vcf):
        write_vcf(vcf, sh["S"], sh["N"])
    evals = sh["S"] * sh["N"]
    print(f"shape {name}: {sh['S']} x {sh['N']} = {evals:.3e} evaluations ({sh['flags']})", flush=True)
    if os.environ.get("PILEUP_RATE_WRITE_ONLY"):
        continue
    piles = []
    for dev in (0, 1):
        out = os.path.join(d, f"o_{name}{dev}")
        argv = [BIN, "-i", vcf, "-o", out, "--verbose", "1", "--device-pileup", str(dev)] + sh["flags"].split()
        t0 = time.perf_counter()
        r = subprocess.run(argv, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-800:]
        with open(out + ".pileup.gz", "rb") as f:
            piles.append(f.read())
        print(f"  --device-pileup {dev}: {dt:7.2f} s  {evals / dt:10.3e} evals/s  pileup {len(piles[-1]) / 1e6:8.1f} MB", flush=True)
        print("    " + [l for l in r.stderr.splitlines() if l.startswith("[timing]")][-1], flush=True)
        os.remove(out + ".pileup.gz")
        os.remove(out + ".bcf")
    assert piles[0] == piles[1], f"shape {name}: --device-pileup 1 wrote another .pileup.gz"
    print("  same .pileup.gz bytes", flush=True)
