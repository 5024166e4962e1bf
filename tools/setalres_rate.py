#!/usr/bin/env python3
"""End-to-end time of setalleles_hip on a BGZF file of BCF with its input read by zlib (--device-inflate 0), with its BGZF members
inflated on the device (--device-inflate 1) and with the file left in GPU memory, its records relabelled, assembled and compressed
there (--device-inflate 1 --resident 1), on files vcfgl_hip writes: SITES x SAMPLES, C3 flags (depth 20, -e 0.01, --error-qs 2,
--beta-variance 1e-5, -GL 2) with -doUnobserved 4 -addPL 1 -addGP 1 -addQS 1, -O b; the TSV cuts every record to REF + 2 ALTs; the
program runs with -O b --threads 16 --on-device 1.
SETALRES_PARENT=dir adds the program of the parent commit (dir/setalleles_hip; it takes no new flag) as a setting of its own.
Everything is inside the measured wall time, process start included.  The settings alternate, SETALRES_REPS times each (default 3),
and are reported as min / median / max with the program's [input] and [setalleles] lines of every run (the stage split of the resident
path is in the latter); all settings of a row must decompress to the same bytes, and the range of --device-inflate 0 is held against
the parent's.
usage (GPU box): python tools/setalres_rate.py [SITESxSAMPLES ...]      (default: 4096x1000 1048576x1 32768x1000)"""
import gzip, hashlib, os, shutil, struct, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import numpy as np
BINDIR = os.path.join(ROOT, "vcfgl_amd", "bin")
PARENT = os.environ.get("SETALRES_PARENT", "")
VCFGL = os.path.join(BINDIR, "vcfgl_hip")
reps = int(os.environ.get("SETALRES_REPS", "3"))
rows = [tuple(int(x) for x in a.split("x")) for a in (sys.argv[1:] or ["4096x1000", "1048576x1", "32768x1000"])]
d = tempfile.mkdtemp(prefix="setalresrate")
C3 = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2 -doUnobserved 4 -addPL 1 -addGP 1 -addQS 1"
NEW, RES = ["--device-inflate", "1"], ["--device-inflate", "1", "--resident", "1"]


def digest(path):
    h = hashlib.sha1()
    with gzip.open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def simulate(S, N):
    src = os.path.join(d, "in.vcf")
    rng = np.random.default_rng(42)
    tok = np.array(["0|0", "1|0", "0|1", "1|1"])
    with open(src, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1))
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n")
        for i in range(S):
            f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (i + 1) + "\t".join(tok[rng.integers(0, 4, N)]) + "\n")
    out = os.path.join(d, "sal")
    r = subprocess.run([VCFGL, "-i", src, "-o", out, "-O", "b"] + C3.split(), capture_output=True, text=True, timeout=1100)
    assert r.returncode == 0, r.stderr[-800:]
    os.remove(src)
    print(f"input -O b: {S} records x {N} samples, {os.path.getsize(out + '.bcf') / 1e6:.1f} MB on disk", flush=True)
    return out + ".bcf"


def typed(f):
    b = f.read(1)[0]
    t, n = b & 15, b >> 4
    if n == 15:
        t2, _ = typed(f)
        n = struct.unpack({1: "<b", 2: "<h", 3: "<i"}[t2], f.read({1: 1, 2: 2, 3: 4}[t2]))[0]
    return t, n


def alleles_tsv(path):
    """REF + 2 ALTs of every record, from its shared block's typed strings"""
    tsv, inflated = os.path.join(d, "alleles.tsv"), 0
    with gzip.open(path, "rb") as f, open(tsv, "w") as g:
        assert f.read(5) == b"BCF\x02\x02"
        f.read(struct.unpack("<I", f.read(4))[0])
        while True:
            head = f.read(8)
            if len(head) < 8:
                break
            l_shared, l_indiv = struct.unpack("<II", head)
            chrom, pos, rlen, qual, nai, nfs = struct.unpack("<iiiIII", f.read(24))
            t, n = typed(f)
            used = 25 + (2 if n >= 15 else 0) + n
            f.read(n)
            names = []
            for _ in range(nai >> 16):
                t, n = typed(f)
                used += 1 + (2 if n >= 15 else 0) + n
                names.append(f.read(n).decode())
            f.seek(l_shared - used + l_indiv, 1)
            inflated += 8 + l_shared + l_indiv
            g.write(names[0] + "\t" + ",".join(names[1:3]) + "\n")
    print(f"  {inflated / 1e6:.1f} MB of records inflated", flush=True)
    return tsv


for S, N in rows:
    path = simulate(S, N)
    tsv = alleles_tsv(path)
    build = lambda exe, out, extra: [exe, "-i", path, "-a", tsv, "-O", "b", "-o", out, "--threads", "16", "--on-device", "1", "--verbose", "1"] + extra
    exe = os.path.join(BINDIR, "setalleles_hip")
    settings = {}
    if PARENT:
        settings["parent commit"] = lambda out: build(os.path.join(PARENT, "setalleles_hip"), out, [])
    settings["--device-inflate 0"] = lambda out: build(exe, out, [])
    settings["--device-inflate 1"] = lambda out: build(exe, out, NEW)
    settings["--device-inflate 1 --resident 1"] = lambda out: build(exe, out, RES)
    print(f"setalleles_hip, {S} x {N}, -O b file, -O b --threads 16 --on-device 1:", flush=True)
    times, digests = {k: [] for k in settings}, {}
    for rep in range(reps):
        for k, cmd in settings.items():
            out = os.path.join(d, "out_" + "".join(c for c in k if c.isalnum()))
            t0 = time.perf_counter()
            r = subprocess.run(cmd(out), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=1100)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-800:]
            times[k].append(dt)
            print(f"  {k} run {rep}: {dt:7.3f} s", flush=True)
            for l in r.stderr.splitlines():
                if l.startswith(("[input]", "[setalleles]")):
                    print("      " + l.replace(d + os.sep, ""), flush=True)
            if rep == 0:
                digests[k] = digest(out + ".bcf")
            os.remove(out + ".bcf")
    assert len(set(digests.values())) == 1, "the settings decompress to different bytes: %r" % digests
    print("  every setting decompresses to the same bytes", flush=True)
    for k, ts in times.items():
        print(f"  {k:36s} min {min(ts):7.3f} s  median {sorted(ts)[len(ts) // 2]:7.3f} s  max {max(ts):7.3f} s", flush=True)
    if PARENT:
        a, b = times["parent commit"], times["--device-inflate 0"]
        print("  --device-inflate 0 against the parent commit: " + ("ranges overlap" if max(min(a), min(b)) <= min(max(a), max(b)) else "below" if max(b) < min(a) else "above"), flush=True)
    os.remove(path)

shutil.rmtree(d, ignore_errors=True)
