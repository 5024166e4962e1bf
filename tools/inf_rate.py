#!/usr/bin/env python3
"""End-to-end rate of the host program with --depth inf on a synthetic input of SITES x SAMPLES phased binary genotypes
(tools/cli_rate.py's input), -addGP 1 -addPL 1 beside the default GL.  Everything is inside the measured wall time: process start,
input parsing, the records, encoding, compression and the file.  Per output the settings alternate, INF_REPS times each (default 3),
and are reported as min / median / max (the protocol of DESIGN 4.15):
    parent   INF_PARENT_BIN=path: another build of the program (one that does not know the flag), the host's --depth inf path
    inf-0    this build with --device-inf 0: the same host path; its range has to overlap the parent's
    inf-1    this build with --device-inf 1 and (a) -O v --device-text 1, (b) -O b --device-bcf 1 --device-stream 1 --device-bgzf 1
The files of the first repetition must hold the same records (all but the ##source= lines).  The last inf-1 run prints its --verbose 1
stage split.  INF_PROFILE=dir: per output one more inf-1 run under `rocprofv3 --kernel-trace --stats` (with INF_REPS=0: a pass of
its own), its kernel_stats rows printed and its files left in dir.
usage (GPU box): [INF_PARENT_BIN=...] [INF_PROFILE=dir] python tools/inf_rate.py [sites] [samples]     INF_OUTPUTS=v,b selects the outputs"""
import glob, gzip, hashlib, os, shutil, struct, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
d = tempfile.mkdtemp(prefix="infrate")
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
print(f"input: {S} sites x {N} samples, {os.path.getsize(vcf) / 1e6:.1f} MB of VCF text", flush=True)
flags = "--seed 42 --depth inf -e 0.01 -addGP 1 -addPL 1".split() + os.environ.get("INF_EXTRA", "").split()
DEVICE = {"v": ["--device-text", "1"], "b": ["--device-bcf", "1", "--device-stream", "1", "--device-bgzf", "1"]}
EXT = {"v": ".vcf", "b": ".bcf"}


def digest(fn, mode):
    """sha1 of the file's content without its ##source= lines, streamed"""
    h = hashlib.sha1()
    if mode == "v":
        with open(fn, "rb") as f:
            for ln in f:
                if not ln.startswith(b"##source="):
                    h.update(ln)
        return h.hexdigest()
    with gzip.open(fn, "rb") as f:                              # (BGZF is a series of gzip members)
        head = f.read(9)
        text = f.read(struct.unpack("<I", head[5:9])[0])
        h.update(b"\n".join(ln for ln in text.split(b"\n") if not ln.startswith(b"##source=")))
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


parent = os.environ.get("INF_PARENT_BIN")
reps = int(os.environ.get("INF_REPS", "3"))
for mode in os.environ.get("INF_OUTPUTS", "v,b").split(","):
    settings = ([("parent", parent, [])] if parent else []) + [("inf-0", BIN, ["--device-inf", "0"]), ("inf-1", BIN, ["--device-inf", "1"] + DEVICE[mode])]
    times, digests, last_err = {k: [] for k, _, _ in settings}, {}, {}
    print(f"\n-O {mode}; inf-1 = --device-inf 1 {' '.join(DEVICE[mode])}", flush=True)
    for rep in range(reps):
        for k, (name, prog, extra) in enumerate(settings):
            out = os.path.join(d, f"o{k}")
            t0 = time.perf_counter()
            r = subprocess.run([prog, "-i", vcf, "-o", out, "-O", mode, "--verbose", "1"] + flags + extra, capture_output=True, text=True)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-800:]
            times[name].append(dt)
            last_err[name] = r.stderr
            size = os.path.getsize(out + EXT[mode]) / 1e6
            print(f"{name:8s} run {rep}: {dt:7.2f} s  {S * N / dt:10.3e} samples x sites/s  records {size:8.1f} MB", flush=True)
            if rep == 0:
                digests[name] = digest(out + EXT[mode], mode)
            os.remove(out + EXT[mode])
    prof = os.environ.get("INF_PROFILE")
    if prof:
        os.makedirs(prof, exist_ok=True)
        out = os.path.join(d, "op")
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "inf_" + mode, "--", BIN, "-i", vcf, "-o", out, "-O", mode,
                            "--device-inf", "1"] + DEVICE[mode] + flags, capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, VCFGL_HIP_NORMAL_EXIT="1"))        # (the program leaves through exit(), so that the profiler writes its files)
        assert r.returncode == 0, r.stderr[-1500:]
        os.remove(out + EXT[mode])
        for fn in sorted(glob.glob(os.path.join(prof, "**", "inf_" + mode + "_kernel_stats.csv"), recursive=True)):
            print(f"\n{fn}:\n" + open(fn).read(), flush=True)
    if reps == 0:
        continue
    assert len(set(digests.values())) == 1, digests
    print(f"\n| -O {mode} | seconds min / median / max | samples x sites/s (median) |\n|---|---|---|")
    for name, _, _ in settings:
        t = sorted(times[name])
        print(f"| {name} | {t[0]:.2f} / {t[len(t) // 2]:.2f} / {t[-1]:.2f} | {S * N / t[len(t) // 2]:.1e} |")
    if parent:
        a, b = sorted(times["parent"]), sorted(times["inf-0"])
        print("\nflag-off range overlaps the parent's:", "yes" if a[0] <= b[-1] and b[0] <= a[-1] else "NO")
    print("\nstage split of the last inf-1 run:")
    print("\n".join(ln for ln in last_err["inf-1"].splitlines() if ln.startswith(("[timing]", "[device"))), flush=True)
shutil.rmtree(d, ignore_errors=True)
