#!/usr/bin/env python3
"""End-to-end time of setalleles_hip with the GL / PL / GP vectors reordered, normalised and narrowed on the host and on the device
(--on-device 0 / 1), on the BCF file that vcfgl_hip writes: SITES x SAMPLES, C3 flags (depth 20, -e 0.01, --error-qs 2,
--beta-variance 1e-5, -GL 2) with -doUnobserved 4 -addPL 1 -addGP 1 -addQS 1, -O b in and -O b out (--threads 16).  The TSV cuts every
record to REF + 2 ALTs.  Everything is inside the measured wall time: process start, reading and inflating the file, the shared blocks,
the vectors, the new records and their BGZF members.  The two settings alternate, SETAL_REPS times each (default 3), and are reported
as min / median / max with the program's [setalleles] line (counts, bytes and stage split) of every run; redone must be 0 and both
settings must write the same decompressed stream.  (VCF text is worked on the host alone: there is nothing to compare.)
usage (GPU box): python tools/setalhip_rate.py [sites] [samples]"""
import gzip, hashlib, os, re, shutil, struct, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import numpy as np
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "setalleles_hip")
VCFGL = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
reps = int(os.environ.get("SETAL_REPS", "3"))
d = tempfile.mkdtemp(prefix="setalrate")
C3 = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2 -doUnobserved 4 -addPL 1 -addGP 1 -addQS 1"

src = os.path.join(d, "in.vcf")
rng = np.random.default_rng(42)
tok = np.array(["0|0", "1|0", "0|1", "1|1"])
with open(src, "w") as f:
    f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1))
    f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n")
    for i in range(S):
        f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (i + 1) + "\t".join(tok[rng.integers(0, 4, N)]) + "\n")
sim = os.path.join(d, "sim")
r = subprocess.run([VCFGL, "-i", src, "-o", sim, "-O", "b"] + C3.split(), capture_output=True, text=True, timeout=1100)
assert r.returncode == 0, r.stderr[-800:]
files = {"b": sim + ".bcf"}
print(f"input -O b: {S} records x {N} samples, {os.path.getsize(files['b']) / 1e6:.1f} MB on disk", flush=True)
os.remove(src)


def typed(f):
    """a typed value's (type, count) at the stream's place"""
    b = f.read(1)[0]
    t, n = b & 15, b >> 4
    if n == 15:
        t2, _ = typed(f)
        n = struct.unpack({1: "<b", 2: "<h", 3: "<i"}[t2], f.read({1: 1, 2: 2, 3: 4}[t2]))[0]
    return t, n


tsv = os.path.join(d, "alleles.tsv")
with gzip.open(files["b"], "rb") as f, open(tsv, "w") as g:             # the alleles of every record: its shared block's typed strings
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
        f.read(l_shared - used + l_indiv)
        g.write(names[0] + "\t" + ",".join(names[1:3]) + "\n")


def cmd(path, mode, on_device, prefix):
    return [BIN, "-i", path, "-a", tsv, "-O", mode, "-o", prefix, "--threads", "16", "--on-device", str(on_device), "--verbose", "1"]


handed_back = {}
for mode, path in files.items():
    ext = ".vcf.gz" if mode == "z" else ".bcf"
    print(f"-O {mode}:", flush=True)
    times, digests = {0: [], 1: []}, {}
    for rep in range(reps):
        for k in (0, 1):
            prefix = os.path.join(d, "o%d" % k)
            t0 = time.perf_counter()
            r = subprocess.run(cmd(path, mode, k, prefix), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=1100)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-800:]
            times[k].append(dt)
            line = [l for l in r.stderr.splitlines() if l.startswith("[setalleles]")][0]
            print(f"  on-device {k} run {rep}: {dt:7.3f} s  {S * N / dt:10.3e} samples/s\n      {line}", flush=True)
            m = re.search(r"records (\d+), redone on the host (\d+)", line)
            assert int(m.group(1)) == S
            if int(m.group(2)):                                         # reported, the run goes on; the tool's exit status says so at the end
                handed_back[mode] = int(m.group(2))
            if rep == 0:
                h = hashlib.sha1()
                with gzip.open(prefix + ext, "rb") as f:
                    for chunk in iter(lambda: f.read(1 << 24), b""):
                        h.update(chunk)
                digests[k] = h.hexdigest()
    assert digests[0] == digests[1], "the two settings wrote different streams"
    print("  both settings wrote the same decompressed stream", flush=True)
    for k, ts in times.items():
        print(f"  on-device {k}  min {min(ts):.3f} s  median {sorted(ts)[len(ts) // 2]:.3f} s  max {max(ts):.3f} s", flush=True)
    lo, hi = max(min(times[0]), min(times[1])), min(max(times[0]), max(times[1]))
    print("  --on-device 1 against 0: " + ("ranges overlap" if lo <= hi else "below" if max(times[1]) < min(times[0]) else "above"), flush=True)

shutil.rmtree(d, ignore_errors=True)
for mode, n in handed_back.items():
    print(f"-O {mode}: {n} of {S} records were handed back to the host (redone must be 0)", flush=True)
sys.exit(1 if handed_back else 0)
