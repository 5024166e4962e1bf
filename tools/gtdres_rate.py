#!/usr/bin/env python3
"""End-to-end time of gtdiscordance_hip with both files of the pair resident in GPU memory (--resident 1) against the staged paths, on
synthetic BGZF pairs of SITES x SAMPLES genotypes (seeded).  Everything is inside the measured wall time: process start, reading both
files, the first nine columns (the heads) and the merge, the comparison, the output.  A row is one pair -- the BGZF text pair of
tools/gtdisc_rate.py (GT:DP:GQ, -doGQ 6) or a BGZF BCF pair of tools/gtdbcf_rate.py (GT:GQ under -doGQ 6, GT:PL under -doGQ 8, with
--bcf-direct 1 throughout); its settings alternate, GTDRES_REPS times each (default 3), and are reported as min / median / max:
    parent        the program of the parent commit (GTDRES_PARENT=path; left out when unset), default flags
    di 0          this program, --device-inflate 0
    di 1          --device-inflate 1
    resident      --device-inflate 1 --resident 1
    per-sample    (BCF rows, GTDRES_NOWIDE=path: this program built with -DGTD_NO_WIDE_ANY, `make -C vcfgl_amd/csrc ../bin/gtdiscordance_hip_nowide`) --device-inflate 1 --resident 1 with
                  unaligned GT vectors read a sample a lane: k_gtd_bcf_decode with and without the any-address wide form
Every setting of a row must write the same bytes.  The [input], [gtdisc], [bcf] and [resident] lines of every run are printed: the
stage split, and under --resident 1 the device stage of the batches and the parse / decode share from hipEvent pairs.
GTDRES_ROWS=text,GQ,PL picks rows.
usage (GPU box): python tools/gtdres_rate.py [sites] [samples]"""
import hashlib, os, re, shutil, struct, subprocess, sys, tempfile, time, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "gtdiscordance_hip")
PARENT, NOWIDE = os.environ.get("GTDRES_PARENT"), os.environ.get("GTDRES_NOWIDE")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
REPS = int(os.environ.get("GTDRES_REPS", "3"))
ROWS = os.environ.get("GTDRES_ROWS", "text,GQ,PL").split(",")
d = tempfile.mkdtemp(prefix="gtdresrate")
rng = np.random.default_rng(42)


class Bgzf:
    """a BGZF writer: members of 65280 bytes at level 1, the empty member at the end"""
    def __init__(self, path):
        self.f, self.buf, self.raw = open(path, "wb"), bytearray(), 0

    def member(self, chunk):
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = z.compress(bytes(chunk)) + z.flush()
        self.f.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(bytes(chunk)), len(chunk)))

    def write(self, data):
        self.buf += data
        self.raw += len(data)
        while len(self.buf) >= 65280:
            self.member(self.buf[:65280])
            del self.buf[:65280]

    def close(self):
        if self.buf:
            self.member(self.buf)
        self.member(b"")
        self.f.close()


def bcf_header(extra):
    lines = ["##fileformat=VCFv4.2", '##FILTER=<ID=PASS,Description="All filters passed",IDX=0>', "##contig=<ID=chr1,length=%d,IDX=0>" % (2 * S + 1),
             '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype",IDX=1>'] + extra
    text = ("\n".join(lines + ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N))]) + "\n").encode() + b"\0"
    return b"BCF\x02\x02" + struct.pack("<I", len(text)) + text


def bcf_record(pos, fields):
    shared = struct.pack("<iiiIII", 0, pos - 1, 1, 0x7F800001, (2 << 16), (len(fields) << 24) | N) + b"\x17.\x17A\x17C\x11\x00"
    indiv = b"".join(bytes([0x11, key, (n << 4) | t]) + data for key, t, n, data in fields)
    return struct.pack("<II", len(shared), len(indiv)) + shared + indiv


files = {}
if "text" in ROWS:
    files["text"] = (os.path.join(d, "truth.vcf.gz"), os.path.join(d, "call.vcf.gz"))
    ft, fc = Bgzf(files["text"][0]), Bgzf(files["text"][1])
    gts = np.array(["%d%s%d" % (a, s, b) for a in range(2) for b in range(2) for s in "/|"])
    head = "##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (2 * S + 1)
    cols = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n"
    ft.write((head + cols).encode())
    fc.write((head + "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"d\">\n##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"q\">\n" + cols).encode())
    nums = np.array([str(i) for i in range(128)])
    pos = 0
    for i in range(S):
        pos += 1
        if rng.random() < 0.1:                              # a truth record the call file lacks
            ft.write(("chr1\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t" % pos + "\t".join(gts[rng.integers(0, 8, N)]) + "\n").encode())
            pos += 1
        t = rng.integers(0, 8, N)
        c = np.where(rng.random(N) < 0.9, t, rng.integers(0, 8, N))
        ft.write(("chr1\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t" % pos + "\t".join(gts[t]) + "\n").encode())
        tok = np.char.add(np.char.add(np.char.add(gts[c], ":"), np.char.add(nums[rng.integers(0, 40, N)], ":")), nums[rng.integers(1, 128, N)])
        tok[rng.random(N) < 0.02] = "./.:0:."
        fc.write(("chr1\t%d\t.\tA\tC\t50\tPASS\t.\tGT:DP:GQ\t" % pos + "\t".join(tok) + "\n").encode())
    ft.close(); fc.close()
    print(f"input: text pair: truth {ft.raw / 1e6:.1f} MB and call {fc.raw / 1e6:.1f} MB of VCF text, {os.path.getsize(files['text'][0]) / 1e6:.1f} + {os.path.getsize(files['text'][1]) / 1e6:.1f} MB as BGZF", flush=True)
if "GQ" in ROWS or "PL" in ROWS:
    rng = np.random.default_rng(42)
    paths = {k: os.path.join(d, k + ".gz.bcf") for k in ("truth", "GQ", "PL")}
    w = {k: Bgzf(p) for k, p in paths.items()}
    w["truth"].write(bcf_header([]))
    w["GQ"].write(bcf_header(['##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="q",IDX=2>']))
    w["PL"].write(bcf_header(['##FORMAT=<ID=PL,Number=G,Type=Integer,Description="p",IDX=2>']))
    pos = 0
    for i in range(S):
        pos += 1
        if rng.random() < 0.1:                              # a truth record the call file lacks
            w["truth"].write(bcf_record(pos, [(1, 1, 2, (2 + 2 * rng.integers(0, 2, 2 * N, dtype=np.int8)).tobytes())]))
            pos += 1
        t = rng.integers(0, 2, (N, 2), dtype=np.int8)
        c = np.where(rng.random((N, 1)) < 0.9, t, rng.integers(0, 2, (N, 2), dtype=np.int8))
        phase = rng.integers(0, 2, (N, 2), dtype=np.int8); phase[:, 0] = 0
        cg = (2 + 2 * c) | phase
        cg[rng.random(N) < 0.02] = 0                        # ./.
        w["truth"].write(bcf_record(pos, [(1, 1, 2, ((2 + 2 * t) | phase).astype(np.int8).tobytes())]))
        gq = rng.integers(1, 128, N, dtype=np.int16).astype(np.int8)
        pl = rng.integers(1, 256, (N, 3), dtype=np.int16); pl[np.arange(N), rng.integers(0, 3, N)] = 0
        w["GQ"].write(bcf_record(pos, [(1, 1, 2, cg.astype(np.int8).tobytes()), (2, 1, 1, gq.tobytes())]))
        w["PL"].write(bcf_record(pos, [(1, 1, 2, cg.astype(np.int8).tobytes()), (2, 2, 3, pl.astype("<i2").tobytes())]))
    for k in w:
        w[k].close()
        print(f"input: {k}: {w[k].raw / 1e6:.1f} MB of BCF, {os.path.getsize(paths[k]) / 1e6:.1f} MB as BGZF", flush=True)
    files["GQ"], files["PL"] = (paths["truth"], paths["GQ"]), (paths["truth"], paths["PL"])
print(f"{S} call records x {N} samples; {REPS} runs a setting, alternating", flush=True)

env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "vcfgl_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
overlap = lambda a, b: max(min(a), min(b)) <= min(max(a), max(b))
for row, mode in (("text", "6"), ("GQ", "6"), ("PL", "8")):
    if row not in ROWS:
        continue
    base = [] if row == "text" else ["--bcf-direct", "1"]
    settings = ([("parent", PARENT, base)] if PARENT else []) + [("di 0", BIN, base + ["--device-inflate", "0"]), ("di 1", BIN, base + ["--device-inflate", "1"]),
                                                              ("resident", BIN, base + ["--device-inflate", "1", "--resident", "1"])]
    if NOWIDE and row != "text":
        settings.append(("per-sample", NOWIDE, base + ["--device-inflate", "1", "--resident", "1"]))
    print(f"== {'BGZF text pair GT:DP:GQ' if row == 'text' else 'BGZF BCF pair, call file GT:' + row}, -doGQ {mode} ==", flush=True)
    times, digests, share = {s[0]: [] for s in settings}, {}, {s[0]: [] for s in settings}
    for rep in range(REPS):
        for name, exe, flags in settings:
            out = os.path.join(d, "o.tsv")
            argv = [exe, "-t", files[row][0], "-i", files[row][1], "-o", out, "-doGQ", mode, "--verbose", "1"] + flags
            t0 = time.perf_counter()
            r = subprocess.run(argv, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-800:]
            times[name].append(dt)
            print(f"{name:11s} run {rep}: {dt:7.3f} s", flush=True)
            for ln in r.stderr.splitlines():
                if ln.startswith(("[input]", "[gtdisc]", "[bcf]", "[resident]")):
                    print("    " + ln.replace(d + "/", ""), flush=True)
            if "--resident" in flags:
                assert r.stderr.count(": resident 1,") == 2, "a file of the pair was not resident"
                m = re.search(r"\[resident\].*device stage ([0-9.]+) ms over (\d+) batches \(hipEvent pairs\), of which (\w+) ([0-9.]+) ms", r.stderr)
                assert " redone on the host 0," in r.stderr and m, "plain records were handed back"
                share[name].append((float(m.group(1)), int(m.group(2)), m.group(3), float(m.group(4))))
            digests.setdefault(name, hashlib.sha1(open(out, "rb").read()).hexdigest())
    assert len(set(digests.values())) == 1, "the settings wrote different bytes: %r" % digests
    for name, ts in times.items():
        print(f"  {name:11s} min {min(ts):.3f} s  median {sorted(ts)[len(ts) // 2]:.3f} s  max {max(ts):.3f} s", flush=True)
    for name, xs in share.items():
        if xs:
            k = sorted(x[3] for x in xs)
            print(f"  {name:11s} device stage {sorted(x[0] for x in xs)[len(xs) // 2]:.3f} ms over {xs[0][1]} batches at the median run; {xs[0][2]} min {k[0]:.3f} ms  median {k[len(k) // 2]:.3f} ms  max {k[-1]:.3f} ms", flush=True)
    if PARENT:
        print("  di 0 against parent: " + ("ranges overlap" if overlap(times["parent"], times["di 0"]) else "RANGES DO NOT OVERLAP"), flush=True)
    a, b = times["di 1"], times["resident"]
    print("  resident against di 1: " + ("ranges overlap" if overlap(a, b) else "below (faster)" if max(b) < min(a) else "ABOVE (slower)"), flush=True)
    a = times["di 0"]
    print("  resident against di 0: " + ("ranges overlap" if overlap(a, b) else "below (faster)" if max(b) < min(a) else "ABOVE (slower)"), flush=True)
shutil.rmtree(d, ignore_errors=True)
