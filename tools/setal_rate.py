#!/usr/bin/env python3
"""End-to-end rate of the host program with --set-alleles on a synthetic input of SITES x SAMPLES phased binary genotypes
(tools/cli_rate.py's input and flags, plus -doUnobserved 4 so that every record has an allele list worth changing).  Everything is
inside the measured wall time: process start, input parsing, the allele file, simulation, relabelling, encoding, compression and the
file.  The settings alternate, SETAL_REPS times each (default 3), and are reported as min / median / max:
    parent       SETAL_PARENT_BIN=path: another build of the program (one that does not know the flag)
    plain        this build, the same flags: the default path must not pay for the feature (its range has to overlap the parent's)
    set-alleles  the same with --set-alleles FILE (every record: A, then C and <*>)
The parent's and the plain run's files must be the same stream but for their ##source= lines.  The last flagged run prints its
--verbose 1 stage split.  For the two kernels' own times run the flagged command once more under
`rocprofv3 --kernel-trace --stats -- <command>` (a run of its own) and keep the k_setal_* rows in profiles/setal_ab/.
usage (GPU box): python tools/setal_rate.py [sites] [samples]"""
import hashlib, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import bcf_reader
import synth
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
d = tempfile.mkdtemp(prefix="setalrate")
vcf, tsv = os.path.join(d, "in.vcf"), os.path.join(d, "alleles.tsv")
gt = synth.binary_sites(0, S, N)
tok = np.array(["0|0", "1|0", "0|1", "1|1"])
with open(vcf, "w") as f:
    f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1))
    f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n")
    for i in range(S):
        g = gt[i]
        idx = (g & 0xF).astype(np.int64) + 2 * (g >> 4).astype(np.int64)
        f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (i + 1) + "\t".join(tok[idx]) + "\n")
with open(tsv, "w") as f:
    f.write("A\tC,<*>\n" * S)
print(f"input: {S} sites x {N} samples, {os.path.getsize(vcf) / 1e6:.1f} MB of VCF text")
flags = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2 -doUnobserved 4".split() + os.environ.get("SETAL_EXTRA", "").split()
rec = ["-O", "b", "--device-bcf", "1", "--device-stream", "1", "--device-bgzf", "1"]


def bcf_digest(fn):
    r = bcf_reader.Reader(fn)
    h = hashlib.sha1("\n".join(x for x in r.header if not x.startswith("##source=")).encode())
    h.update(r.raw[r.off:])
    return h.hexdigest()


parent = os.environ.get("SETAL_PARENT_BIN")
settings = ([("parent", parent, rec)] if parent else []) + [("plain", BIN, rec), ("set-alleles", BIN, rec + ["--set-alleles", tsv])]
times, digests, last_err = {k: [] for k, _, _ in settings}, {}, {}
for rep in range(int(os.environ.get("SETAL_REPS", "3"))):
    for k, (name, prog, extra) in enumerate(settings):
        out = os.path.join(d, f"o{k}")
        t0 = time.perf_counter()
        r = subprocess.run([prog, "-i", vcf, "-o", out, "--verbose", "1"] + flags + extra, capture_output=True, text=True)
        dt = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-800:]
        times[name].append(dt)
        last_err[name] = r.stderr
        size = os.path.getsize(out + ".bcf") / 1e6
        print(f"{name:12s} run {rep}: {dt:7.2f} s  {S * N / dt:10.3e} evals/s  records {size:8.1f} MB", flush=True)
        if rep == 0 and name != "set-alleles":
            digests[name] = bcf_digest(out + ".bcf")
assert len(set(digests.values())) <= 1, digests
print("\n| setting | seconds min / median / max | evaluations/s (median) |\n|---|---|---|")
for name, _, _ in settings:
    t = sorted(times[name])
    print(f"| {name} | {t[0]:.2f} / {t[len(t) // 2]:.2f} / {t[-1]:.2f} | {S * N / t[len(t) // 2]:.1e} |")
if parent:
    a, b = sorted(times["parent"]), sorted(times["plain"])
    print("\nflag-off range overlaps the parent's:", "yes" if a[0] <= b[-1] and b[0] <= a[-1] else "NO")
print("\nstage split of the last 'set-alleles' run:")
print("\n".join(ln for ln in last_err["set-alleles"].splitlines() if ln.startswith(("[timing]", "[device"))))
