#!/usr/bin/env python3
"""End-to-end time of fetchgl_hip with the sample columns read on the host and on the device (--on-device 0 / 1), on record files that
vcfgl_hip writes: SITES x SAMPLES, C3 flags (depth 20, -e 0.01, --error-qs 2, --beta-variance 1e-5, -GL 2), once as -O z (bgzip'd VCF
text) and once as -O b (bgzip'd BCF).  Everything is inside the measured wall time: process start, reading and inflating the file, the
first nine columns, the values, the CSV (-o FILE) and the tool's per-record messages.  The two settings alternate, FETCHGL_REPS times
each (default 3), and are reported as min / median / max with the program's [fetchgl] line (counts, bytes and stage split) of every
run.  Both settings must write the same bytes.  Then one more --on-device 1 run per file under rocprofv3 --kernel-trace --stats (a
run of its own, never timed end to end): the per-batch times of the kernels, and k_fgl_parse's GB/s of text (the bytes the program
reports as sent up over the kernel's total time).
FETCHGL_GT=AC (default), FETCHGL_PROFILE=dir keeps the kernel statistics there.
usage (GPU box): python tools/fetchglhip_rate.py [sites] [samples]"""
import csv, glob, hashlib, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import numpy as np
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "fetchgl_hip")
VCFGL = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
gt = os.environ.get("FETCHGL_GT", "AC")
reps = int(os.environ.get("FETCHGL_REPS", "3"))
d = tempfile.mkdtemp(prefix="fetchglrate")
C3 = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2"

src = os.path.join(d, "in.vcf")
rng = np.random.default_rng(42)
tok = np.array(["0|0", "1|0", "0|1", "1|1"])
with open(src, "w") as f:
    f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1))
    f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n")
    for i in range(S):
        f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (i + 1) + "\t".join(tok[rng.integers(0, 4, N)]) + "\n")
files = {}
for mode, ext in (("z", ".vcf.gz"), ("b", ".bcf")):
    out = os.path.join(d, "sim_" + mode)
    r = subprocess.run([VCFGL, "-i", src, "-o", out, "-O", mode] + C3.split(), capture_output=True, text=True, timeout=1100)
    assert r.returncode == 0, r.stderr[-800:]
    files[mode] = out + ext
    print(f"input -O {mode}: {S} records x {N} samples, {os.path.getsize(files[mode]) / 1e6:.1f} MB on disk", flush=True)
os.remove(src)


def cmd(path, on_device, out):
    return [BIN, "-i", path, "-gt", gt, "-o", out, "--on-device", str(on_device), "--verbose", "1"]


for mode, path in files.items():
    print(f"-O {mode}, -gt {gt}:", flush=True)
    times, digests, up = {0: [], 1: []}, {}, 0
    for rep in range(reps):
        for k in (0, 1):
            out = os.path.join(d, "o%d.csv" % k)
            t0 = time.perf_counter()
            r = subprocess.run(cmd(path, k, out), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=1100)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-800:]
            times[k].append(dt)
            line = [l for l in r.stderr.splitlines() if l.startswith("[fetchgl]")][0]
            print(f"  on-device {k} run {rep}: {dt:7.3f} s  {S * N / dt:10.3e} values/s\n      {line}", flush=True)
            m = re.search(r"records (\d+), with a CSV line (\d+), redone on the host (\d+), bytes sent up (\d+)", line)
            assert int(m.group(1)) == S and int(m.group(3)) == 0, "records were handed back"
            if k == 1:
                up = int(m.group(4))
            if rep == 0:
                digests[k] = hashlib.sha1(open(out, "rb").read() + r.stderr.split("[fetchgl]")[0].encode()).hexdigest()
                lines, size = int(m.group(2)), os.path.getsize(out)
    assert digests[0] == digests[1], "the two settings wrote different bytes"
    print(f"  {lines} CSV lines, {size / 1e6:.1f} MB; both settings wrote the same CSV and messages", flush=True)
    for k, ts in times.items():
        print(f"  on-device {k}  min {min(ts):.3f} s  median {sorted(ts)[len(ts) // 2]:.3f} s  max {max(ts):.3f} s  {S * N / sorted(ts)[len(ts) // 2]:.3e} values/s at the median", flush=True)
    lo, hi = max(min(times[0]), min(times[1])), min(max(times[0]), max(times[1]))
    print("  --on-device 1 against 0: " + ("ranges overlap" if lo <= hi else "below" if max(times[1]) < min(times[0]) else "above"), flush=True)

    prof = os.path.join(os.environ.get("FETCHGL_PROFILE") or os.path.join(d, "prof"), "O" + mode)
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "fetchgl", "--"] + cmd(path, 1, os.path.join(d, "p.csv")),
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=1100)
    assert r.returncode == 0, r.stderr[-800:]
    stats = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
    assert stats, "rocprofv3 wrote no kernel statistics"
    for row in csv.DictReader(open(stats[0])):
        if "k_fgl_" not in row["Name"] and "k_offsets_scan" not in row["Name"]:
            continue
        name = re.search(r"k_fgl_\w+|k_offsets_scan", row["Name"]).group(0)
        line = f"  {name:12s} {int(row['Calls']):5d} batches  average {float(row['AverageNs']) / 1e3:9.1f} us  min {int(row['MinNs']) / 1e3:9.1f}  max {int(row['MaxNs']) / 1e3:9.1f}  total {int(row['TotalDurationNs']) / 1e6:8.3f} ms"
        if name in ("k_fgl_parse", "k_fgl_pick"):
            line += f"  {up / int(row['TotalDurationNs']):.1f} GB/s of what was sent up"
        print(line, flush=True)
shutil.rmtree(d, ignore_errors=True)
