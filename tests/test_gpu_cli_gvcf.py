"""vcfgl_hip --device-gvcf 1 (gVCF blocks built and the sample columns formatted on the device, blocks that cross a tile merged on the
host) writes the files --device-gvcf 0 writes: seeded random gVCF inputs over tile sizes that make blocks cross tiles and fill whole
tiles, two contexts, sites removed by --rm-empty-sites, several contigs, 1 to 500 samples, -addQS, the pileup, -O v and -O z with and
without --device-bgzf 1 (compared decompressed: the ##source line names the flag); and the reference's golden gVCF outputs again with --device-gvcf 1."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(gu.REFVCF, "data")


def run(argv):
    r = subprocess.run([BIN] + argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.mark.parametrize("name", ["test7", "test8", "test19"])
def test_golden_gvcf_outputs_with_device_gvcf(name, tmp_path):
    t = gu.REF_TESTS[name]
    assert "-doGVCF 1" in t["args"]
    out = str(tmp_path / name)
    run(["-i", os.path.join(DATA, t["input"]), "-o", out, "--rng-mode", "1", "--device-gvcf", "1"] + t["args"].split())
    ours = [l.rstrip("\n") for l in open(out + ".vcf") if not l.startswith("##")]
    gold = [l.rstrip("\n") for l in open(os.path.join(gu.REFVCF, "reference", name, name + ".vcf")) if not l.startswith("##")]
    assert ours == gold


def random_vcf(rng, path, N, contigs):
    """runs of hom-ref sites over several contigs with a few variable records"""
    with open(path, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n")
        rows = []
        for c in range(contigs):
            length = int(rng.integers(20, 400))
            fh.write(f"##contig=<ID=chr{c + 1},length={length}>\n")
            pos = np.sort(rng.choice(np.arange(1, length + 1), size=int(rng.integers(1, min(length, 12) + 1)), replace=False))
            rows += [(f"chr{c + 1}", int(p)) for p in pos]
        fh.write("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        fh.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(f"s{i}" for i in range(N)) + "\n")
        for chrom, p in rows:
            a = ["0", "1"]                                                  # (the binary GT source, --source 0)
            gts = ["0|0"] * N if rng.random() < 0.7 else [f"{rng.integers(0, 2)}|{rng.integers(0, 2)}" for _ in range(N)]
            fh.write(f"{chrom}\t{p}\t.\t{a[0]}\t{a[1]}\t.\tPASS\t.\tGT\t" + "\t".join(gts) + "\n")


def body(path):
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rb") as f:
        return [l for l in f.read().split(b"\n") if not l.startswith(b"##source=")]


CASES = []
for k in range(12):
    CASES.append(dict(seed=8100 + k, N=[1, 2, 65, 500][k % 4], tile=[7, 64, 4096][k % 3], devices=(k % 5 == 1), rm_empty=(k % 2 == 0),
                      qs=(k % 3 != 1), pileup=(k % 4 == 1), mode=["v", "z", "z-bgzf"][k % 3]))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_random_gvcf_runs_equal_the_host_blocker(case, tmp_path):
    c = CASES[case]
    rng = np.random.default_rng(c["seed"])
    inp = str(tmp_path / "in.vcf")
    random_vcf(rng, inp, c["N"], contigs=int(rng.integers(1, 4)))
    depth = 2.0 if c["pileup"] else 12.0 if c["N"] >= 65 else float(rng.choice([3.0, 12.0]))
    dps = sorted({1} | set(int(x) for x in rng.integers(2, 12, int(rng.integers(0, 4)))))       # (1: a site with reads in every sample can block)
    err = 0.0 if c["N"] >= 65 else float(rng.choice([0.0, 0.001]))
    m = c["mode"][0]
    argv = ["-i", inp, "-O", m, "--seed", str(c["seed"]), "--depth", str(depth), "--error-rate", str(err),
            "-explode", "1", "-doUnobserved", str(int(rng.choice([1, 2]))), "-addPL", "1", "-doGVCF", "1", "--gvcf-dps", ",".join(map(str, dps)),
            "--tile-sites", str(c["tile"]), "-addQS", str(int(c["qs"])), "--rm-empty-sites", str(int(c["rm_empty"])),
            "-printPileup", str(int(c["pileup"]))]
    if c["devices"]:
        argv += ["--devices", "0,0"]
    if c["mode"] == "z-bgzf":
        argv += ["--device-bgzf", "1"]
    ext = ".vcf" if m == "v" else ".vcf.gz"
    a, b = str(tmp_path / "host"), str(tmp_path / "dev")
    run(argv + ["-o", a])
    rb = run(argv + ["-o", b, "--device-gvcf", "1"])
    ba, bb = body(a + ext), body(b + ext)
    assert ba == bb
    assert len(ba) > 10
    assert any(b"MIN_DP=" in l for l in ba)
    if c["pileup"]:
        assert gzip.open(a + ".pileup.gz").read() == gzip.open(b + ".pileup.gz").read()
    assert "Number of sites included" in rb.stderr
