#!/usr/bin/env python3
"""End-to-end time of gtdiscordance_hip with the comparison on the host and on the device (--on-device 0 / 1), on a synthetic truth /
call pair of SITES x SAMPLES genotypes (FORMAT GT:DP:GQ, seeded).  Everything is inside the measured wall time: process start,
reading both files, the first nine columns and the merge, the comparison, the output.  The two settings alternate, GTDISC_REPS times
each (default 3), and are reported as min / median / max with the program's [gtdisc] line (counts and stage split) of every run.
Both settings must write the same bytes.  Then one more --on-device 1 run under rocprofv3 --kernel-trace --stats (a run of its
own, never timed end to end): the per-batch times of the four kernels and k_gtd_parse's GB/s of text (the bytes the program reports
as sent up over the kernel's total time).
GTDISC_MODE=6 (default; any -doGQ 0 .. 8), GTDISC_PERSITE=1 adds -perSite 1, GTDISC_PROFILE=dir keeps the kernel statistics there.
usage (GPU box): python tools/gtdisc_rate.py [sites] [samples]"""
import csv, glob, hashlib, os, re, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import numpy as np
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "gtdiscordance_hip")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
mode = os.environ.get("GTDISC_MODE", "6")
per_site = os.environ.get("GTDISC_PERSITE", "0")
d = tempfile.mkdtemp(prefix="gtdiscrate")
truth, call = os.path.join(d, "truth.vcf"), os.path.join(d, "call.vcf")
rng = np.random.default_rng(42)
gts = np.array(["%d%s%d" % (a, s, b) for a in range(2) for b in range(2) for s in "/|"])
head = "##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (2 * S + 1)
cols = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n"
with open(truth, "w") as ft, open(call, "w") as fc:
    ft.write(head + cols)
    fc.write(head + "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"d\">\n##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"q\">\n" + cols)
    nums = np.array([str(i) for i in range(128)])
    pos = 0
    for i in range(S):
        pos += 1
        if rng.random() < 0.1:                              # a truth record the call file lacks
            ft.write("chr1\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t" % pos + "\t".join(gts[rng.integers(0, 8, N)]) + "\n")
            pos += 1
        t = rng.integers(0, 8, N)
        c = np.where(rng.random(N) < 0.9, t, rng.integers(0, 8, N))
        ft.write("chr1\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t" % pos + "\t".join(gts[t]) + "\n")
        tok = np.char.add(np.char.add(np.char.add(gts[c], ":"), np.char.add(nums[rng.integers(0, 40, N)], ":")), nums[rng.integers(1, 128, N)])
        tok[rng.random(N) < 0.02] = "./.:0:."
        fc.write("chr1\t%d\t.\tA\tC\t50\tPASS\t.\tGT:DP:GQ\t" % pos + "\t".join(tok) + "\n")
print(f"input: {S} call records x {N} samples, truth {os.path.getsize(truth) / 1e6:.1f} MB and call {os.path.getsize(call) / 1e6:.1f} MB of VCF text; -doGQ {mode}, -perSite {per_site}", flush=True)


def cmd(on_device, out):
    return [BIN, "-t", truth, "-i", call, "-o", out, "-doGQ", mode, "-perSite", per_site, "--on-device", str(on_device), "--verbose", "1"]


times, digests, up = {0: [], 1: []}, {}, 0
for rep in range(int(os.environ.get("GTDISC_REPS", "3"))):
    for k in (0, 1):
        out = os.path.join(d, "o%d.tsv" % k)
        t0 = time.perf_counter()
        with open(os.path.join(d, "stdout%d" % k), "wb") as so:
            r = subprocess.run(cmd(k, out), stdout=so, stderr=subprocess.PIPE, text=True, timeout=1100)
        dt = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-800:]
        times[k].append(dt)
        line = [l for l in r.stderr.splitlines() if l.startswith("[gtdisc]")][0]
        print(f"on-device {k} run {rep}: {dt:7.3f} s  {S * N / dt:10.3e} calls/s\n    {line}", flush=True)
        if k == 1:
            m = re.search(r"records (\d+), redone on the host (\d+), text bytes sent up (\d+)", line)
            assert int(m.group(1)) == S and int(m.group(2)) == 0, "the device handed plain records back"
            up = int(m.group(3))
        if rep == 0:
            h = hashlib.sha1(open(out, "rb").read())
            h.update(open(os.path.join(d, "stdout%d" % k), "rb").read())
            digests[k] = h.hexdigest()
assert digests[0] == digests[1], "the two settings wrote different bytes"
for k, ts in times.items():
    print(f"  on-device {k}  min {min(ts):.3f} s  median {sorted(ts)[len(ts) // 2]:.3f} s  max {max(ts):.3f} s  {S * N / sorted(ts)[len(ts) // 2]:.3e} calls/s at the median", flush=True)
lo, hi = max(min(times[0]), min(times[1])), min(max(times[0]), max(times[1]))
print("  --on-device 1 against 0: " + ("ranges overlap" if lo <= hi else "below" if max(times[1]) < min(times[0]) else "above"), flush=True)

prof = os.environ.get("GTDISC_PROFILE") or os.path.join(d, "prof")
r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "gtdisc", "--"] + cmd(1, os.path.join(d, "p.tsv")),
                   stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=1100)
assert r.returncode == 0, r.stderr[-800:]
stats = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
assert stats, "rocprofv3 wrote no kernel statistics"
for row in csv.DictReader(open(stats[0])):
    if "k_gtd_" not in row["Name"] and "k_offsets_scan" not in row["Name"]:
        continue
    name = re.search(r"k_gtd_\w+|k_offsets_scan", row["Name"]).group(0)
    line = f"  {name:18s} {int(row['Calls']):5d} batches  average {float(row['AverageNs']) / 1e3:9.1f} us  min {int(row['MinNs']) / 1e3:9.1f}  max {int(row['MaxNs']) / 1e3:9.1f}  total {int(row['TotalDurationNs']) / 1e6:8.3f} ms"
    if name == "k_gtd_parse":
        line += f"  {up / int(row['TotalDurationNs']):.1f} GB/s of text"
    print(line, flush=True)
shutil.rmtree(d, ignore_errors=True)
