#!/usr/bin/env python3
"""End-to-end rate of `vcfgl_hip -doGVCF 1` with the host blocker (--device-gvcf 0) and the device blocker (--device-gvcf 1), for -O v
and for -O z --device-bgzf 1, on three shapes:
  a  one sample, one hom-ref contig exploded (-explode 1) over POSITIONS positions, depth 10, -e 0.001, --gvcf-dps 1,5,10,20: long blocks
  b  C5 flags (-doUnobserved 2, depth 5, -e 0.01) on 262144 sites x 500 samples: nearly every site is a record
  c  1000 samples, depth 30, -e 0, --gvcf-dps 10,12,14,16: short blocks that alternate
Everything is inside the wall time (process start, input parsing, PCIe, encoding, compression); the program's own [timing] line follows.
Both settings must write the same body (the ##source line names the flag): checked on every pair.
GVCF_RATE_BCF=1 measures the binary modes instead: -O u and -O b --device-bgzf 1, --device-gvcf 0 --device-bcf 0 (the host blocker, whose
blocks go through a text line) against --device-gvcf 1 --device-bcf 1; the decompressed streams must be equal but for ##source=.
usage (GPU box): python tools/gvcf_rate.py [shapes, e.g. abc] [POSITIONS]
GVCF_RATE_DIR=dir keeps the inputs there (in_<shape>.vcf); GVCF_RATE_WRITE_ONLY=1 writes them and prints each shape's flags, e.g. for
a profiler run of one vcfgl_hip process (with VCFGL_HIP_NORMAL_EXIT=1, so that the profiler's exit handlers run)."""
import gzip, hashlib, os, struct, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
SHAPES = sys.argv[1] if len(sys.argv) > 1 else "abc"
POSITIONS = int(sys.argv[2]) if len(sys.argv) > 2 else 4_000_000
d = os.environ.get("GVCF_RATE_DIR") or tempfile.mkdtemp(prefix="gvcfrate")
os.makedirs(d, exist_ok=True)


def write_vcf(path, S, N, length, hom_ref):
    gt = synth.binary_sites(0, S, N)
    tok = np.array(["0|0", "1|0", "0|1", "1|1"])
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=%d>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" % length)
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("ind%d" % i for i in range(N)) + "\n")
        row0 = "\t".join(["0|0"] * N)
        for i in range(S):
            pos = (i + 1) * (length // S) if hom_ref else i + 1
            if hom_ref:
                row = row0
            else:
                g = gt[i]
                row = "\t".join(tok[(g & 0xF).astype(np.int64) + 2 * (g >> 4).astype(np.int64)])
            f.write("chr1\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t%s\n" % (pos, row))


shapes = {
    "a": dict(S=16, N=1, length=POSITIONS, hom_ref=True, evals=POSITIONS,
              flags="--depth 10 -e 0.001 -explode 1 -doUnobserved 2 -addPL 1 -doGVCF 1 --gvcf-dps 1,5,10,20"),
    "b": dict(S=262144, N=500, length=262145, hom_ref=False, evals=262144 * 500,
              flags="--depth 5 -e 0.01 -doUnobserved 2 -addPL 1 -doGVCF 1 --gvcf-dps 1,3,5"),
    "c": dict(S=32768, N=1000, length=32769, hom_ref=True, evals=32768 * 1000,
              flags="--depth 30 -e 0 -doUnobserved 2 -addPL 1 -doGVCF 1 --gvcf-dps 10,12,14,16"),
}
for name in SHAPES:
    sh = shapes[name]
    vcf = os.path.join(d, f"in_{name}.vcf")
    write_vcf(vcf, sh["S"], sh["N"], sh["length"], sh["hom_ref"])
    print(f"shape {name}: {sh['evals']:.3e} evaluations ({sh['flags']})", flush=True)
    if os.environ.get("GVCF_RATE_WRITE_ONLY"):
        continue
    BCF = bool(os.environ.get("GVCF_RATE_BCF"))
    for mode, extra in ((("u", []), ("b", ["--device-bgzf", "1"])) if BCF else (("v", []), ("z", ["--device-bgzf", "1"]))):
        bodies = []
        for dev in (0, 1):
            out = os.path.join(d, f"o_{name}{mode}{dev}")
            argv = [BIN, "-i", vcf, "-o", out, "-O", mode, "--seed", "42", "--verbose", "1", "--device-gvcf", str(dev)] + extra + sh["flags"].split()
            if BCF:
                argv += ["--device-bcf", str(dev)]
            t0 = time.perf_counter()
            r = subprocess.run(argv, capture_output=True, text=True)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr[-800:]
            fn = out + (".bcf" if BCF else ".vcf" if mode == "v" else ".vcf.gz")
            if BCF:                                                     # the stream without the ##source= lines of its header
                with (gzip.open if mode == "b" else open)(fn, "rb") as f:
                    raw = f.read()
                l_text = struct.unpack_from("<I", raw, 5)[0]
                hdr = b"\n".join(l for l in raw[9:9 + l_text].split(b"\n") if not l.startswith(b"##source="))
                bodies.append(hashlib.sha1(hdr + raw[9 + l_text:]).hexdigest())
                print(f"  -O {mode} {' '.join(extra):16s} --device-gvcf {dev} --device-bcf {dev}: {dt:7.2f} s  {sh['evals'] / dt:10.3e} evals/s  "
                      f"{os.path.getsize(fn) / 1e6:8.1f} MB", flush=True)
                for l in r.stderr.splitlines():
                    if l.startswith("[device"):
                        print("    " + l, flush=True)
            else:
                with (gzip.open if mode == "z" else open)(fn, "rb") as f:
                    body = [l for l in f.read().split(b"\n") if not l.startswith(b"##source=")]
                bodies.append(body)
                n_blk = sum(1 for l in body if b"MIN_DP=" in l)
                print(f"  -O {mode} {' '.join(extra):16s} --device-gvcf {dev}: {dt:7.2f} s  {sh['evals'] / dt:10.3e} evals/s  "
                      f"{len(body) - 1} lines, {n_blk} blocks, {os.path.getsize(fn) / 1e6:8.1f} MB", flush=True)
            print("    " + [l for l in r.stderr.splitlines() if l.startswith("[timing]")][-1], flush=True)
            os.remove(fn)
        assert bodies[0] == bodies[1], f"shape {name} -O {mode}: the device settings wrote other bytes"
