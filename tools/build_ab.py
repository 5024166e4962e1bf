#!/usr/bin/env python3
"""Two builds of the project against each other on one machine, alternating, with identical flags: the front end's wall time per
output row (as tools/cli_rate.py measures it: process start to file written), its `device context(s)` time from the [timing] line,
and the headline of `python bench.py --gpus 1`.  For a change that is meant to leave speed alone (a refactor of host code).

usage (GPU box): python tools/build_ab.py PARENT_DIR [sites] [samples]
PARENT_DIR holds the other build as bin/vcfgl_hip and lib/libvcfgl_hip.so (a copy of vcfgl_amd/bin and vcfgl_amd/lib made at that
commit).  AB_REPS runs of each build per row (default 5); AB_AA=1 puts a copy of THIS build in the parent's place (the A/A control:
what the rotation's second place costs by itself); AB_BENCH=0 skips bench.py, AB_CLI=0 the front end."""
import json, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth

parent = os.path.abspath(sys.argv[1])
S = int(sys.argv[2]) if len(sys.argv) > 2 else 32768
N = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
REPS = int(os.environ.get("AB_REPS", "5"))
d = tempfile.mkdtemp(prefix="buildab")
if os.environ.get("AB_AA"):
    for sub in ("bin", "lib"):
        shutil.copytree(os.path.join(ROOT, "vcfgl_amd", sub), os.path.join(d, "aa", sub))
    parent = os.path.join(d, "aa")
builds = [("parent" if not os.environ.get("AB_AA") else "copy", parent), ("this", os.path.join(ROOT, "vcfgl_amd"))]


def summary(name, ts, unit="s"):
    ts = sorted(ts)
    print(f"  {name:8s} min {ts[0]:.4g} {unit}  median {ts[len(ts) // 2]:.4g} {unit}  max {ts[-1]:.4g} {unit}", flush=True)


if os.environ.get("AB_CLI", "1") != "0":
    vcf = os.path.join(d, "in.vcf")
    gt = synth.binary_sites(0, S, N)
    tok = np.array(["0|0", "1|0", "0|1", "1|1"])
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1))
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n")
        for i in range(S):
            idx = (gt[i] & 0xF).astype(np.int64) + 2 * (gt[i] >> 4).astype(np.int64)
            f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (i + 1) + "\t".join(tok[idx]) + "\n")
    print(f"input: {S} sites x {N} samples, {os.path.getsize(vcf) / 1e6:.1f} MB of VCF text")
    flags = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2 --verbose 1".split()
    rows = [("-O u", ["-O", "u"]), ("--device-stream 1 -O b", ["-O", "b", "--device-bgzf", "1", "--device-bcf", "1", "--device-stream", "1"])]
    for row, extra in rows:
        wall, ctx, sizes = {b: [] for b, _ in builds}, {b: [] for b, _ in builds}, set()
        for rep in range(REPS):
            for b, where in builds:
                out = os.path.join(d, "out")
                t0 = time.perf_counter()
                r = subprocess.run([os.path.join(where, "bin", "vcfgl_hip"), "-i", vcf, "-o", out] + extra + flags, capture_output=True, text=True, timeout=120)
                dt = time.perf_counter() - t0
                assert r.returncode == 0, r.stderr[-800:]
                m = re.search(r"device context\(s\) ([0-9.]+) s", r.stderr)
                wall[b].append(dt)
                ctx[b].append(float(m.group(1)))
                sizes.add(os.path.getsize(out + ".bcf"))
                print(f"{row:24s} {b:8s} run {rep}: {dt:7.3f} s  {S * N / dt:10.3e} evals/s  device context(s) {m.group(1)} s", flush=True)
                os.remove(out + ".bcf")
        assert len(sizes) == 1, f"{row}: the builds wrote files of different sizes"
        for b, _ in builds:
            summary(b, wall[b])
        for b, _ in builds:
            summary(b, ctx[b], "s context")

if os.environ.get("AB_BENCH", "1") != "0":
    vals = {b: [] for b, _ in builds}
    for rep in range(REPS):
        for b, where in builds:
            env = dict(os.environ, VGL_LIB=os.path.join(where, "lib", "libvcfgl_hip.so"))
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
            assert r.returncode == 0, r.stderr[-800:]
            line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            vals[b].append(float(line["value"]))
            print(f"bench.py {b:8s} run {rep}: {line.get('metric', 'value')} = {line['value']:.5g} {line.get('unit', '')}  ({time.perf_counter() - t0:.0f} s)", flush=True)
    for b, _ in builds:
        summary(b, vals[b], "")
shutil.rmtree(d, ignore_errors=True)
