#!/usr/bin/env python3
"""Process start to finish of fetchgl_hip --on-device 1 on a file of 3 samples x 5 records: another build's binary
(MISCSTART_OTHER=dir/fetchgl_hip, e.g. the parent commit's) and this tree's, alternating, 15 runs each after a first pair that is not
counted -- what a larger binary costs outside every stage timer.
usage (GPU box): MISCSTART_OTHER=path python tools/miscstart_rate.py"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import fgl_file_model as gm
import tempfile
d = tempfile.mkdtemp(prefix="miscstart")
path = gm.write_file(os.path.join(d, "tiny.bgz"), gm.make_records(3, 5, seed=1, fixed_alleles=True), 3, "bgz")
exes = {"parent commit": os.environ["MISCSTART_OTHER"], "this commit": os.path.join(ROOT, "vcfgl_amd", "bin", "fetchgl_hip")}
times = {k: [] for k in exes}
for rep in range(16):
    for k, exe in exes.items():
        t0 = time.perf_counter()
        r = subprocess.run([exe, "-i", path, "-gt", "AC", "-o", os.path.join(d, "tiny.csv"), "--on-device", "1"], capture_output=True, timeout=60)
        dt = time.perf_counter() - t0
        if r.returncode != 0:
            print("STOP", k, r.returncode); sys.exit(1)
        if rep:                                            # the first pair warms the page cache
            times[k].append(dt)
for k, ts in times.items():
    ts.sort()
    print(f"{k:14s} 15 runs  min {ts[0]:.4f} s  median {ts[7]:.4f} s  max {ts[-1]:.4f} s", flush=True)
for k, exe in exes.items():
    print(f"{k:14s} {os.path.getsize(exe)} bytes")
