#!/usr/bin/env python3
"""End-to-end time of the host program on BCF input with the genotypes decoded on the host and on the device (--device-bcf-input 0 / 1),
on a synthetic BCF of SITES x SAMPLES phased binary genotypes as int8 pairs (tools/input_rate.py's genotypes and flags, alleles A, C
read with --source 1).  Everything is inside the measured wall time: process start, reading and decoding the input, simulation, and
-- where records are written -- encoding, assembly, compression and the file.  The settings alternate, BCFIN_REPS times each
(default 3), and are reported as min / median / max, with the [timing] line of the first run and the [input] lines of every run of each:
    parent    BCFIN_PARENT_BIN=path: another build of the program (one that does not know the flag)
    bcf 0     --device-bcf-input 0
    bcf 1     --device-bcf-input 1
BCFIN_INPUT=raw (default): the BCF as it is; BCFIN_INPUT=bgzf: as BGZF members (zlib level 1, 0xff00 bytes each) with --device-inflate 1
in every setting.  BCFIN_MODE=table (default): --records 0 --gt-discordance 1; BCFIN_MODE=records: -O b --device-bcf 1 --device-stream 1
--device-bgzf 1 with the tally.  Every setting must write the same table and, with records, the same decompressed stream but for its
##source= lines.  The --device-bcf-input 0 range must overlap the parent's (the split of the reader costs nothing).
BCFIN_PROFILE=dir: one more run of --device-bcf-input 1 under rocprofv3 --kernel-trace --stats (a pass of its own): k_bcfin_decode's time
per batch and its rate of genotype bytes from the trace.
usage (GPU box): [BCFIN_MODE=records] [BCFIN_INPUT=bgzf] [BCFIN_PARENT_BIN=...] [BCFIN_PROFILE=dir] python tools/bcfin_rate.py [sites] [samples]"""
import csv, glob, gzip, hashlib, os, shutil, struct, subprocess, sys, tempfile, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
mode, kind = os.environ.get("BCFIN_MODE", "table"), os.environ.get("BCFIN_INPUT", "raw")
d = tempfile.mkdtemp(prefix="bcfinrate")
bcf = os.path.join(d, "in.bcf")


def bgzf_member(data):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(data), len(data)))


header = ("##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\",IDX=0>\n##contig=<ID=chr1,length=%d,IDX=0>\n"
          "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\",IDX=1>\n" % (S + 1)
          + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n\0").encode()
pending = bytearray()
with open(bcf, "wb") as f:
    def put(b, last=False):
        if kind != "bgzf":
            f.write(b)
            return
        pending.extend(b)
        while len(pending) >= 0xff00 or (last and pending):
            f.write(bgzf_member(bytes(pending[:0xff00])))
            del pending[:0xff00]
    put(b"BCF\x02\x02" + struct.pack("<I", len(header)) + header)
    # shared block: chr1, pos, rlen 1, QUAL missing, two alleles, no INFO, one FORMAT field; ID ".", REF A, ALT C, FILTER PASS
    tail = struct.pack("<iIII", 1, 0x7F800001, 2 << 16, (1 << 24) | N) + b"\x17.\x17A\x17C\x11\x00"
    indiv_head = bytes([0x11, 1, 0x21])                                  # key GT, two int8 per sample
    for s0 in range(0, S, 4096):                                         # (in blocks: the generator's tables grow with the block)
        gt = synth.binary_sites(s0, min(4096, S - s0), N)
        vals = np.empty(gt.shape + (2,), np.uint8)
        vals[:, :, 0] = ((gt & 0xF) + 1) << 1
        vals[:, :, 1] = (((gt >> 4) + 1) << 1) | 1
        block = []
        for i in range(gt.shape[0]):
            shared = struct.pack("<ii", 0, s0 + i) + tail
            block.append(struct.pack("<II", len(shared), 3 + 2 * N) + shared + indiv_head + vals[i].tobytes())
        put(b"".join(block))
    put(b"", last=True)
    if kind == "bgzf":
        f.write(bgzf_member(b""))
print(f"input: {S} sites x {N} samples, {os.path.getsize(bcf) / 1e6:.1f} MB of {'BGZF ' if kind == 'bgzf' else ''}BCF; mode {mode}", flush=True)
flags = "--seed 42 --depth 20 -e 0.01 --error-qs 2 --beta-variance 1e-5 -GL 2 --source 1".split() + os.environ.get("BCFIN_EXTRA", "").split()
flags += ["--device-inflate", "1"] if kind == "bgzf" else []
out_flags = (["-O", "b", "--device-bcf", "1", "--device-stream", "1", "--device-bgzf", "1", "--gt-discordance", "1", "--discordance-gq", "6"]
             if mode == "records" else ["--records", "0", "--gt-discordance", "1", "--discordance-gq", "6"])


def bcf_digest(fn):
    """sha1 of a BCF stream without the ##source= lines of its header"""
    raw = gzip.decompress(open(fn, "rb").read())
    l_text = struct.unpack_from("<I", raw, 5)[0]
    h = hashlib.sha1(b"\n".join(l for l in raw[9:9 + l_text].split(b"\n") if not l.startswith(b"##source=")))
    h.update(memoryview(raw)[9 + l_text:])
    return h.hexdigest()


parent = os.environ.get("BCFIN_PARENT_BIN")
settings = ([("parent", parent, [])] if parent else []) + [("bcf 0", BIN, ["--device-bcf-input", "0"]), ("bcf 1", BIN, ["--device-bcf-input", "1"])]
times, digests, tables = {k: [] for k, _, _ in settings}, {}, {}
for rep in range(int(os.environ.get("BCFIN_REPS", "3"))):
    for k, (name, prog, extra) in enumerate(settings):
        out = os.path.join(d, f"o{k}")
        t0 = time.perf_counter()
        r = subprocess.run([prog, "-i", bcf, "-o", out, "--verbose", "1"] + flags + out_flags + extra, capture_output=True, text=True, timeout=600)
        dt = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr[-800:]
        times[name].append(dt)
        print(f"{name:8s} run {rep}: {dt:7.3f} s  {S * N / dt:10.3e} evals/s", flush=True)
        for l in r.stderr.splitlines():                  # the stage split of every run: the start-up of the runtime varies from run to run
            if (l.startswith("[timing]") and rep == 0) or l.startswith("[input]"):
                print("    " + l, flush=True)
        if name == "bcf 1":
            assert f"--device-bcf-input 1: {S} records decoded on the device, 0 of them again on the host" in r.stderr, "records were handed back"
        if rep == 0:
            if os.path.exists(out + ".bcf"):
                digests[name] = bcf_digest(out + ".bcf")
            tables[name] = hashlib.sha1(open(out + ".discordance.tsv", "rb").read()).hexdigest()
        for e in (".bcf", ".discordance.tsv"):
            if os.path.exists(out + e):
                os.remove(out + e)
prof = os.environ.get("BCFIN_PROFILE")
if prof:
    os.makedirs(prof, exist_ok=True)
    out = os.path.join(d, "op")
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "bcfin", "--", BIN, "-i", bcf, "-o", out,
                        "--device-bcf-input", "1"] + flags + out_flags, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, VCFGL_HIP_NORMAL_EXIT="1"))        # (the program leaves through exit(), so that the profiler writes its files)
    assert r.returncode == 0, r.stderr[-1500:]
    durs = []
    for fn in glob.glob(os.path.join(prof, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(fn)):
            if "k_bcfin_decode" in row["Kernel_Name"]:
                durs.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    if durs:
        print(f"  k_bcfin_decode: {len(durs)} launches, {sum(durs) / 1e3:.3f} ms in all, median {sorted(durs)[len(durs) // 2]:.1f} us a batch, "
              f"{2.0 * S * N / (sum(durs) * 1e-6) / 1e9:.1f} GB/s of genotype bytes read", flush=True)
shutil.rmtree(d, ignore_errors=True)
assert len(tables) == len(settings) and len(set(tables.values())) == 1, "the settings wrote different tables"
assert len(set(digests.values())) <= 1 and len(digests) == (len(settings) if mode == "records" else 0), "the settings wrote different record streams"
for name, ts in times.items():
    print(f"  {name:8s} min {min(ts):.3f} s  median {sorted(ts)[len(ts) // 2]:.3f} s  max {max(ts):.3f} s  {S * N / sorted(ts)[len(ts) // 2]:.3e} evals/s at the median", flush=True)

if parent:      # the default path pays nothing: its range must overlap the parent's
    lo, hi = max(min(times["parent"]), min(times["bcf 0"])), min(max(times["parent"]), max(times["bcf 0"]))
    print("  --device-bcf-input 0 against the parent: " + ("OVERLAP" if lo <= hi else "NO OVERLAP"), flush=True)
    assert lo <= hi, "the --device-bcf-input 0 range does not overlap the parent's"
lo, hi = max(min(times["bcf 0"]), min(times["bcf 1"])), min(max(times["bcf 0"]), max(times["bcf 1"]))
print("  --device-bcf-input 1 against 0: " + ("ranges overlap" if lo <= hi else "below" if max(times["bcf 1"]) < min(times["bcf 0"]) else "above"), flush=True)
