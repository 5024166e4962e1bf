#!/usr/bin/env python3
"""End-to-end time of the three misc programs with their input read by zlib (--device-inflate 0), with its BGZF members inflated on the
device (--device-inflate 1) and, for fetchgl_hip, with the inflated file left on the device (--device-inflate 1 --resident 1 on VCF
text, and --resident-bcf 1 beside it on BCF), on files vcfgl_hip writes: SITES x SAMPLES, C3 flags (depth 20, -e 0.01, --error-qs 2, --beta-variance 1e-5, -GL 2).
  fetchgl_hip        -O z and -O b files, --on-device 1, -gt AC, -o FILE
  setalleles_hip     the -O b file of a run with -doUnobserved 4 -addPL 1 -addGP 1 -addQS 1, -O b out, --threads 16, --on-device 1; the
                     TSV cuts every record to REF + 2 ALTs
  gtdiscordance_hip  -doGQ 6, --on-device 1, on the synthetic truth / call pair of tools/gtdisc_rate.py written as BGZF
MISCREAD_PARENT=dir adds the programs of the parent commit (dir/fetchgl_hip ...; they take no new flag) as a setting of their own.
Everything is inside the measured wall time, process start included.  The settings alternate, MISCREAD_REPS times each (default 3),
and are reported as min / median / max with the programs' [input] and stage lines of every run; all settings of a row must write the
same bytes.  MISCREAD_ONLY=fetchgl,setal,gtdisc picks programs, MISCREAD_MODES=z,b the files of fetchgl_hip; the mode `short` is a
-O b file of many short records: one sample, MISCREAD_SHORT records (default 2^20).
usage (GPU box): python tools/miscread_rate.py [sites] [samples]"""
import gzip, hashlib, os, shutil, struct, subprocess, sys, tempfile, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import numpy as np
BINDIR = os.path.join(ROOT, "vcfgl_amd", "bin")
PARENT = os.environ.get("MISCREAD_PARENT", "")
VCFGL = os.path.join(BINDIR, "vcfgl_hip")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
reps = int(os.environ.get("MISCREAD_REPS", "3"))
only = os.environ.get("MISCREAD_ONLY", "fetchgl,setal,gtdisc").split(",")
d = tempfile.mkdtemp(prefix="miscreadrate")
C3 = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2"
NEW, RES = ["--device-inflate", "1"], ["--device-inflate", "1", "--resident", "1"]
RES_BCF = RES + ["--resident-bcf", "1"]
SHORT = int(os.environ.get("MISCREAD_SHORT", str(1 << 20)))


def digest(path, inflate):
    h = hashlib.sha1()
    with (gzip.open(path, "rb") if inflate else open(path, "rb")) as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def row(title, settings, out_of, tags, inflate=False):
    """settings: name -> command builder (out) -> argv; alternating runs, the lines of the programs, min / median / max"""
    print(title, flush=True)
    times, digests = {k: [] for k in settings}, {}
    for rep in range(reps):
        for k, build in settings.items():
            out = os.path.join(d, "out_" + "".join(c for c in k if c.isalnum()))
            t0 = time.perf_counter()
            r = subprocess.run(build(out), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=1100)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-800:]
            times[k].append(dt)
            print(f"  {k} run {rep}: {dt:7.3f} s", flush=True)
            for l in r.stderr.splitlines():
                if l.startswith(tags):
                    print("      " + l.replace(d + os.sep, ""), flush=True)
            if rep == 0:
                digests[k] = digest(out_of(out), inflate)
    assert len(set(digests.values())) == 1, "the settings wrote different bytes: %r" % digests
    print("  every setting wrote the same bytes", flush=True)
    for k, ts in times.items():
        print(f"  {k:44s} min {min(ts):7.3f} s  median {sorted(ts)[len(ts) // 2]:7.3f} s  max {max(ts):7.3f} s", flush=True)
    if "parent commit" in times:
        a, b = times["parent commit"], times["--device-inflate 0"]
        print("  --device-inflate 0 against the parent commit: " + ("ranges overlap" if max(min(a), min(b)) <= min(max(a), max(b)) else "below" if max(b) < min(a) else "above"), flush=True)


def simulate(tag, mode, extra="", S=S, N=N):
    src = os.path.join(d, "in.vcf")
    rng = np.random.default_rng(42)
    tok = np.array(["0|0", "1|0", "0|1", "1|1"])
    with open(src, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1))
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n")
        for i in range(S):
            f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (i + 1) + "\t".join(tok[rng.integers(0, 4, N)]) + "\n")
    out = os.path.join(d, tag)
    r = subprocess.run([VCFGL, "-i", src, "-o", out, "-O", mode] + (C3 + " " + extra).split(), capture_output=True, text=True, timeout=1100)
    assert r.returncode == 0, r.stderr[-800:]
    os.remove(src)
    path = out + (".vcf.gz" if mode == "z" else ".bcf")
    print(f"input {tag} -O {mode}: {S} records x {N} samples, {os.path.getsize(path) / 1e6:.1f} MB on disk", flush=True)
    return path


def with_parent(program, settings, build):
    if PARENT:
        settings = dict({"parent commit": lambda out: build(os.path.join(PARENT, program), out, [])}, **settings)
    return settings


if "fetchgl" in only:
    for mode in os.environ.get("MISCREAD_MODES", "z,b").split(","):
        path = simulate("fgl_" + mode, "b", S=SHORT, N=1) if mode == "short" else simulate("fgl_" + mode, mode)
        build = lambda exe, out, extra, path=path: [exe, "-i", path, "-gt", "AC", "-o", out, "--on-device", "1", "--verbose", "1"] + extra
        exe = os.path.join(BINDIR, "fetchgl_hip")
        settings = {"--device-inflate 0": lambda out: build(exe, out, []), "--device-inflate 1": lambda out: build(exe, out, NEW)}
        if mode == "z":
            settings["--device-inflate 1 --resident 1"] = lambda out: build(exe, out, RES)
        else:
            settings["--device-inflate 1 --resident 1 --resident-bcf 1"] = lambda out: build(exe, out, RES_BCF)
        row(f"fetchgl_hip, -O {mode} file, --on-device 1:", with_parent("fetchgl_hip", settings, build), lambda out: out, ("[input]", "[fetchgl]"))
        os.remove(path)

if "setal" in only:
    path = simulate("sal", "b", "-doUnobserved 4 -addPL 1 -addGP 1 -addQS 1")

    def typed(f):
        b = f.read(1)[0]
        t, n = b & 15, b >> 4
        if n == 15:
            t2, _ = typed(f)
            n = struct.unpack({1: "<b", 2: "<h", 3: "<i"}[t2], f.read({1: 1, 2: 2, 3: 4}[t2]))[0]
        return t, n

    tsv = os.path.join(d, "alleles.tsv")
    with gzip.open(path, "rb") as f, open(tsv, "w") as g:               # the alleles of every record: its shared block's typed strings
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
    build = lambda exe, out, extra: [exe, "-i", path, "-a", tsv, "-O", "b", "-o", out, "--threads", "16", "--on-device", "1", "--verbose", "1"] + extra
    exe = os.path.join(BINDIR, "setalleles_hip")
    settings = {"--device-inflate 0": lambda out: build(exe, out, []), "--device-inflate 1": lambda out: build(exe, out, NEW)}
    row("setalleles_hip, -O b file, --on-device 1:", with_parent("setalleles_hip", settings, build), lambda out: out + ".bcf", ("[input]", "[setalleles]"), inflate=True)
    os.remove(path)

if "gtdisc" in only:
    def bgzf_writer(path):
        f = open(path, "wb")
        buf = bytearray()

        def member(chunk):
            z = zlib.compressobj(1, zlib.DEFLATED, -15)
            body = z.compress(chunk) + z.flush()
            f.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(chunk), len(chunk)))

        def write(s):
            buf.extend(s.encode())
            while len(buf) >= 65280:
                member(bytes(buf[:65280]))
                del buf[:65280]

        def close():
            if buf:
                member(bytes(buf))
            member(b"")
            f.close()
        return write, close

    truth, call = os.path.join(d, "truth.vcf.gz"), os.path.join(d, "call.vcf.gz")
    rng = np.random.default_rng(42)
    gts = np.array(["%d%s%d" % (a, s, b) for a in range(2) for b in range(2) for s in "/|"])
    head = "##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (2 * S + 1)
    cols = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n"
    (wt, ct), (wc, cc) = bgzf_writer(truth), bgzf_writer(call)
    wt(head + cols)
    wc(head + "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"d\">\n##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"q\">\n" + cols)
    nums = np.array([str(i) for i in range(128)])
    pos = 0
    for i in range(S):
        pos += 1
        if rng.random() < 0.1:                              # a truth record the call file lacks
            wt("chr1\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t" % pos + "\t".join(gts[rng.integers(0, 8, N)]) + "\n")
            pos += 1
        t = rng.integers(0, 8, N)
        c = np.where(rng.random(N) < 0.9, t, rng.integers(0, 8, N))
        wt("chr1\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t" % pos + "\t".join(gts[t]) + "\n")
        tok = np.char.add(np.char.add(np.char.add(gts[c], ":"), np.char.add(nums[rng.integers(0, 40, N)], ":")), nums[rng.integers(1, 128, N)])
        tok[rng.random(N) < 0.02] = "./.:0:."
        wc("chr1\t%d\t.\tA\tC\t50\tPASS\t.\tGT:DP:GQ\t" % pos + "\t".join(tok) + "\n")
    ct(); cc()
    print(f"input: {S} call records x {N} samples, truth {os.path.getsize(truth) / 1e6:.1f} MB and call {os.path.getsize(call) / 1e6:.1f} MB of BGZF VCF text; -doGQ 6", flush=True)
    build = lambda exe, out, extra: [exe, "-t", truth, "-i", call, "-o", out, "-doGQ", "6", "--on-device", "1", "--verbose", "1"] + extra
    exe = os.path.join(BINDIR, "gtdiscordance_hip")
    settings = {"--device-inflate 0": lambda out: build(exe, out, []), "--device-inflate 1": lambda out: build(exe, out, NEW)}
    row("gtdiscordance_hip -doGQ 6, --on-device 1:", with_parent("gtdiscordance_hip", settings, build), lambda out: out, ("[input]", "[gtdisc]"))

shutil.rmtree(d, ignore_errors=True)
