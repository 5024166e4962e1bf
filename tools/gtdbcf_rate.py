#!/usr/bin/env python3
"""End-to-end time of gtdiscordance_hip on a BCF truth / call pair with and without --bcf-direct 1, on a synthetic pair of SITES x SAMPLES
genotypes (seeded; biallelic records, int8 GT pairs, GQ as int8 or PL as int16 triples).  Everything is inside the measured wall
time: process start, reading both files, the records' notes and the merge, the comparison, the output.  A row is one call file
(GT:GQ under -doGQ 6, GT:PL under -doGQ 8) in one container (raw BCF, BGZF BCF); its settings alternate, GTDBCF_REPS times each
(default 3), and are reported as min / median / max:
    parent        the program of the parent commit (GTDBCF_PARENT=path; left out when unset), default flags
    direct 0      this program, --bcf-direct 0
    direct 1      --bcf-direct 1
    direct 1 +di  --bcf-direct 1 --device-inflate 1
Every setting of a row must write the same bytes.  The [gtdisc] and [bcf] lines of every run are printed: the stage split, the device
stage time from hipEvent pairs, k_gtd_bcf_decode's time per batch and its bytes per second (vector bytes sent up over that time).
GTDBCF_HOST=1 compares on the host instead (--on-device 0, no GPU touched, the device-inflate setting left out).
usage (GPU box): python tools/gtdbcf_rate.py [sites] [samples]"""
import hashlib, os, re, shutil, struct, subprocess, sys, tempfile, time, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "gtdiscordance_hip")
PARENT = os.environ.get("GTDBCF_PARENT")
S = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
N = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
REPS = int(os.environ.get("GTDBCF_REPS", "3"))
d = tempfile.mkdtemp(prefix="gtdbcfrate")
rng = np.random.default_rng(42)


def header(extra):
    lines = ["##fileformat=VCFv4.2", '##FILTER=<ID=PASS,Description="All filters passed",IDX=0>', "##contig=<ID=chr1,length=%d,IDX=0>" % (2 * S + 1),
             '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype",IDX=1>'] + extra
    text = ("\n".join(lines + ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N))]) + "\n").encode() + b"\0"
    return b"BCF\x02\x02" + struct.pack("<I", len(text)) + text


def record(pos, fields):
    shared = struct.pack("<iiiIII", 0, pos - 1, 1, 0x7F800001, (2 << 16), (len(fields) << 24) | N) + b"\x17.\x17A\x17C\x11\x00"
    indiv = b"".join(bytes([0x11, key, (n << 4) | t]) + data for key, t, n, data in fields)
    return struct.pack("<II", len(shared), len(indiv)) + shared + indiv


def bgzf(data, path, block=65280):
    with open(path, "wb") as f:
        for at in list(range(0, len(data), block)) + [len(data)]:
            chunk = data[at:at + block]
            z = zlib.compressobj(1, zlib.DEFLATED, -15)
            body = z.compress(chunk) + z.flush()
            f.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(chunk), len(chunk)))


truth = [header([])]
calls = {"GQ": [header(['##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="q",IDX=2>'])], "PL": [header(['##FORMAT=<ID=PL,Number=G,Type=Integer,Description="p",IDX=2>'])]}
pos = 0
for i in range(S):
    pos += 1
    if rng.random() < 0.1:                                  # a truth record the call file lacks
        truth.append(record(pos, [(1, 1, 2, (2 + 2 * rng.integers(0, 2, 2 * N, dtype=np.int8)).tobytes())]))
        pos += 1
    t = rng.integers(0, 2, (N, 2), dtype=np.int8)
    c = np.where(rng.random((N, 1)) < 0.9, t, rng.integers(0, 2, (N, 2), dtype=np.int8))
    phase = rng.integers(0, 2, (N, 2), dtype=np.int8); phase[:, 0] = 0
    cg = (2 + 2 * c) | phase
    cg[rng.random(N) < 0.02] = 0                            # ./.
    truth.append(record(pos, [(1, 1, 2, ((2 + 2 * t) | phase).astype(np.int8).tobytes())]))
    gq = rng.integers(1, 128, N, dtype=np.int16).astype(np.int8)
    pl = rng.integers(1, 256, (N, 3), dtype=np.int16); pl[np.arange(N), rng.integers(0, 3, N)] = 0
    calls["GQ"].append(record(pos, [(1, 1, 2, cg.astype(np.int8).tobytes()), (2, 1, 1, gq.tobytes())]))
    calls["PL"].append(record(pos, [(1, 1, 2, cg.astype(np.int8).tobytes()), (2, 2, 3, pl.astype("<i2").tobytes())]))
files = {}
for name, parts in (("truth", truth), ("GQ", calls["GQ"]), ("PL", calls["PL"])):
    data = b"".join(parts)
    files[name, "raw"], files[name, "bgzf"] = os.path.join(d, name + ".bcf"), os.path.join(d, name + ".gz.bcf")
    open(files[name, "raw"], "wb").write(data)
    bgzf(data, files[name, "bgzf"])
    print(f"input: {name}: {len(data) / 1e6:.1f} MB of BCF, {os.path.getsize(files[name, 'bgzf']) / 1e6:.1f} MB as BGZF", flush=True)
del truth, calls
print(f"{S} call records x {N} samples; {REPS} runs a setting, alternating", flush=True)

SETTINGS = ([("parent", PARENT, [])] if PARENT else []) + [("direct 0", BIN, ["--bcf-direct", "0"]), ("direct 1", BIN, ["--bcf-direct", "1"]),
                                                          ("direct 1 +di", BIN, ["--bcf-direct", "1", "--device-inflate", "1"])]
if os.environ.get("GTDBCF_HOST") == "1":
    SETTINGS = [(n, e, f + ["--on-device", "0"]) for n, e, f in SETTINGS[:-1]]
env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "vcfgl_amd", "lib") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
for fmt, mode in (("GQ", "6"), ("PL", "8")):
    for container in ("raw", "bgzf"):
        print(f"== call file GT:{fmt}, -doGQ {mode}, {container} BCF ==", flush=True)
        times, digests = {s[0]: [] for s in SETTINGS}, {}
        for rep in range(REPS):
            for name, exe, flags in SETTINGS:
                out = os.path.join(d, "o.tsv")
                argv = [exe, "-t", files["truth", container], "-i", files[fmt, container], "-o", out, "-doGQ", mode, "--verbose", "1"] + flags
                t0 = time.perf_counter()
                r = subprocess.run(argv, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600, env=env)
                dt = time.perf_counter() - t0
                assert r.returncode == 0, r.stderr[-800:]
                times[name].append(dt)
                print(f"{name:13s} run {rep}: {dt:7.3f} s", flush=True)
                for ln in r.stderr.splitlines():
                    if ln.startswith(("[gtdisc]", "[bcf]")):
                        print("    " + ln, flush=True)
                        m = re.search(r"redone on the host (\d+); vector bytes sent up (\d+), text bytes sent up (\d+); device stage ([0-9.]+) ms over (\d+) batches \(hipEvent pairs\), of which k_gtd_bcf_decode ([0-9.]+) ms", ln)
                        if m and float(m.group(6)) > 0:
                            assert int(m.group(1)) == 0, "plain records were handed back"
                            print(f"    k_gtd_bcf_decode: {float(m.group(6)) / int(m.group(5)) * 1e3:.1f} us a batch, {int(m.group(2)) / float(m.group(6)) / 1e6:.1f} GB/s of vectors", flush=True)
                digests.setdefault(name, hashlib.sha1(open(out, "rb").read()).hexdigest())
        assert len(set(digests.values())) == 1, "the settings wrote different bytes: %r" % digests
        for name, ts in times.items():
            print(f"  {name:13s} min {min(ts):.3f} s  median {sorted(ts)[len(ts) // 2]:.3f} s  max {max(ts):.3f} s", flush=True)
        if PARENT:
            a, b = times["parent"], times["direct 0"]
            print("  direct 0 against parent: " + ("ranges overlap" if max(min(a), min(b)) <= min(max(a), max(b)) else "RANGES DO NOT OVERLAP"), flush=True)
        a, b = times["direct 0"], times["direct 1"]
        print("  direct 1 against direct 0: " + ("ranges overlap" if max(min(a), min(b)) <= min(max(a), max(b)) else "below" if max(b) < min(a) else "ABOVE (slower)"), flush=True)
shutil.rmtree(d, ignore_errors=True)
