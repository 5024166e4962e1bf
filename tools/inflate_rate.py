#!/usr/bin/env python3
"""End-to-end time of the host program on a BGZF input inflated by zlib on the host and by the device (--device-inflate 0 / 1), on
tools/input_rate.py's synthetic input of SITES x SAMPLES phased binary genotypes written as BGZF at zlib level 6 (members of 0xff00
bytes and the EOF member: what bgzip writes).  Everything is inside the measured wall time: process start, reading, inflating and
parsing the input, simulation and the discordance table (--records 0 --gt-discordance 1).  For --device-input 0 and for 1 the
settings alternate, INFLATE_REPS times each (default 3), and are reported as min / median / max, with the [input] lines of every run:
    parent     INFLATE_PARENT_BIN=path: another build of the program (one that does not know the flag)
    inflate 0  --device-inflate 0
    inflate 1  --device-inflate 1
Every setting must write the same table.  INFLATE_PROFILE=dir: one more run of --device-inflate 1 under rocprofv3 --kernel-trace
--stats (a pass of its own), k_inflate_member's time per batch and its rate of output from the trace.
usage (GPU box): [INFLATE_PARENT_BIN=...] [INFLATE_PROFILE=dir] python tools/inflate_rate.py [sites] [samples]"""
import csv, glob, hashlib, os, shutil, struct, subprocess, sys, tempfile, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
M = 0xff00
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
d = tempfile.mkdtemp(prefix="inflaterate")
vcf = os.path.join(d, "in.vcf.gz")
tok = np.array(["0|0", "1|0", "0|1", "1|1"])


class Bgzf:
    """a writer of BGZF members at zlib level 6"""
    def __init__(self, path):
        self.f, self.buf, self.n_in, self.n_out, self.members = open(path, "wb"), bytearray(), 0, 0, 0

    def member(self, data):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        dfl = c.compress(data) + c.flush()
        raw = (b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 18 + len(dfl) + 8 - 1) + dfl +
               struct.pack("<II", zlib.crc32(data), len(data)))
        self.f.write(raw); self.n_in += len(data); self.n_out += len(raw); self.members += 1

    def write(self, b):
        self.buf += b
        while len(self.buf) >= M:
            self.member(bytes(self.buf[:M])); del self.buf[:M]

    def close(self):
        if self.buf:
            self.member(bytes(self.buf))
        self.f.write(EOF); self.n_out += len(EOF); self.members += 1
        self.f.close()


w = Bgzf(vcf)
w.write(("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % (S + 1)).encode())
w.write(("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n").encode())
for s0 in range(0, S, 4096):                          # (in blocks: the generator's tables grow with the block)
    gt = synth.binary_sites(s0, min(4096, S - s0), N)
    for i in range(gt.shape[0]):
        g = gt[i]
        idx = (g & 0xF).astype(np.int64) + 2 * (g >> 4).astype(np.int64)
        w.write(("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t" % (s0 + i + 1) + "\t".join(tok[idx]) + "\n").encode())
w.close()
print(f"input: {S} sites x {N} samples, {w.n_in / 1e6:.1f} MB of VCF text in {w.members} BGZF members, {w.n_out / 1e6:.1f} MB compressed (zlib level 6)", flush=True)
flags = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2 --records 0 --gt-discordance 1 --discordance-gq 6".split() + os.environ.get("INFLATE_EXTRA", "").split()
parent = os.environ.get("INFLATE_PARENT_BIN")
reps = int(os.environ.get("INFLATE_REPS", "3"))
tables, rows, ok = set(), [], True
for di in ("0", "1"):
    settings = ([("parent", parent, [])] if parent else []) + [("inflate 0", BIN, ["--device-inflate", "0"]), ("inflate 1", BIN, ["--device-inflate", "1"])]
    times = {k: [] for k, _, _ in settings}
    for rep in range(reps):
        for k, (name, prog, extra) in enumerate(settings):
            out = os.path.join(d, f"o{k}")
            t0 = time.perf_counter()
            r = subprocess.run([prog, "-i", vcf, "-o", out, "--verbose", "1", "--device-input", di] + flags + extra, capture_output=True, text=True, timeout=600)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-800:]
            times[name].append(dt)
            print(f"--device-input {di} {name:9s} run {rep}: {dt:7.3f} s", flush=True)
            for l in r.stderr.splitlines():
                if (l.startswith("[timing]") and rep == 0) or l.startswith("[input]"):
                    print("    " + l, flush=True)
            tables.add(hashlib.sha1(open(out + ".discordance.tsv", "rb").read()).hexdigest())
            os.remove(out + ".discordance.tsv")
    for name, ts in times.items():
        rows.append(f"  --device-input {di} {name:9s} min {min(ts):.3f} s  median {sorted(ts)[len(ts) // 2]:.3f} s  max {max(ts):.3f} s")
    if parent:      # the default path pays nothing: its range must overlap the parent's
        lo, hi = max(min(times["parent"]), min(times["inflate 0"])), min(max(times["parent"]), max(times["inflate 0"]))
        rows.append(f"  --device-input {di}: --device-inflate 0 against the parent: " + ("OVERLAP" if lo <= hi else "NO OVERLAP"))
        ok = ok and lo <= hi
    lo, hi = max(min(times["inflate 0"]), min(times["inflate 1"])), min(max(times["inflate 0"]), max(times["inflate 1"]))
    rows.append(f"  --device-input {di}: --device-inflate 1 against 0: " + ("ranges overlap" if lo <= hi else "below (outside the spread)" if max(times["inflate 1"]) < min(times["inflate 0"]) else "above (outside the spread)"))
print("\n".join(rows), flush=True)
assert len(tables) == 1, "the settings wrote different tables"
print("  every setting wrote the same table", flush=True)

prof = os.environ.get("INFLATE_PROFILE")
if prof:
    os.makedirs(prof, exist_ok=True)
    out = os.path.join(d, "op")
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "inflate", "--", BIN, "-i", vcf, "-o", out, "--device-input", "1",
                        "--device-inflate", "1"] + flags, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, VCFGL_HIP_NORMAL_EXIT="1"))        # (the program leaves through exit(), so that the profiler writes its files)
    assert r.returncode == 0, r.stderr[-1500:]
    durs = []
    for fn in glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(fn)):
            if "k_inflate_member" in row["Kernel_Name"]:
                durs.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    if durs:
        full = sorted(durs)[len(durs) // 2]
        print(f"  k_inflate_member: {len(durs)} launches, {sum(durs) / 1e3:.2f} ms in all, median {full:.0f} us per batch of 512 members; "
              f"{w.n_in / 1e9 / (sum(durs) / 1e6):.2f} GB/s of output over the launches, {w.n_in / (sum(durs) / 1e6) / 1e6 / 512:.1f} MB/s per resident member", flush=True)
    else:
        print("  no k_inflate_member launch in the trace", flush=True)
shutil.rmtree(d, ignore_errors=True)
assert ok, "the --device-inflate 0 range does not overlap the parent's"
