"""vcfgl_hip --device-pileup 1 (the sample columns of -printPileup 1's lines formatted on the device) writes the .pileup.gz that
--device-pileup 0 writes, byte for byte (the BGZF members are the stream's 0xff00-byte cuts either way), and leaves every other output
unchanged: over the quality rules, the GL models, site removal, -explode, -doUnobserved, per-sample depths, every -O mode, the device
BGZF / text / gVCF paths, two contexts, small tiles and both RNG modes.  The reference's golden pileups are reproduced with it."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bcf_reader
import golden_util as gu
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(gu.REFVCF, "data")
DOC = os.path.join(ROOT, "tests", "golden", "doc_error_qs")


def run(argv):
    r = subprocess.run([BIN] + argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pileup_in")
    S, N = 400, 37
    gt = synth.binary_sites(3, S, N)
    tok = np.array(["0|0", "1|0", "0|1", "1|1"])
    vcf = str(d / "in.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=100000>\n##contig=<ID=chr2,length=100000>\n")
        f.write("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("s%d" % i for i in range(N)) + "\n")
        for i in range(S):
            g = gt[i]
            row = "\t".join(tok[(g & 0xF).astype(np.int64) + 2 * (g >> 4).astype(np.int64)])
            f.write("chr%d\t%d\t.\t0\t1\t.\tPASS\t.\tGT\t%s\n" % (1 + (i >= S // 2), 10 + 3 * i, row))
    depths = str(d / "depths.txt")
    with open(depths, "w") as f:
        f.write("\n".join(str(x) for x in np.random.default_rng(1).choice([0.0, 0.4, 3.0, 9.5, 30.0], N)) + "\n")
    return vcf, depths


EQ2 = ["--error-qs", "2", "--beta-variance", "1e-4"]
GV = ["-doGVCF", "1", "--gvcf-dps", "1,3", "-addPL", "1", "-doUnobserved", "2"]
MATRIX = {
    "eq0": ["--error-qs", "0"],
    "eq1": ["--error-qs", "1", "--beta-variance", "1e-4"],
    "eq2": EQ2,
    "gl1": ["-GL", "1", "-addPL", "1"],
    "gl2": ["-GL", "2", "-addGP", "1"],
    "precise": ["--precise-gl", "1"] + EQ2,
    "adj4_eq0": ["--adjust-qs", "4", "--error-qs", "0"],
    "adj4_eq1": ["--adjust-qs", "4", "--error-qs", "1", "--beta-variance", "1e-4"],
    "adj4_eq2": ["--adjust-qs", "4"] + EQ2,
    "adj4_eq2_by": ["--adjust-qs", "4", "--adjust-by", "0.3"] + EQ2,
    "rm_empty": ["--rm-empty-sites", "1", "--depth", "0.4"],
    "rm_invar": ["--rm-invar-sites", "7"],
    "explode": ["-explode", "1", "-doUnobserved", "4"],
    "unobserved": ["-doUnobserved", "2", "-addFormatAD", "1"],
    "depths_file": ["--depths-file", None],
    "O_v": ["-O", "v"],
    "O_z": ["-O", "z"],
    "O_u": ["-O", "u"],
    "O_b_dbgzf": ["-O", "b", "--device-bgzf", "1", "--threads", "4"],
    "O_z_dtext": ["-O", "z", "--device-text", "1", "--device-bgzf", "1", "-addPL", "1"],
    "O_v_dgvcf": ["-O", "v", "--device-gvcf", "1"] + GV,
    "O_z_dgvcf_bgzf": ["-O", "z", "--device-gvcf", "1", "--device-bgzf", "1"] + GV,
    "devices": ["--devices", "0,0", "--tile-sites", "50"],
    "tiles7": ["--tile-sites", "7"],
    "serial": ["--rng-mode", "1"] + EQ2,
    "serial_adj4": ["--rng-mode", "1", "--adjust-qs", "4", "--tile-sites", "64"] + EQ2,
}


def main_output(out, mode):
    """the main output file with the ##source lines left out (they name the flags)"""
    if mode in ("u", "b"):
        rd = bcf_reader.Reader(out + ".bcf")
        return rd.raw[rd.off:]
    fn = out + (".vcf" if mode == "v" else ".vcf.gz")
    with (gzip.open if mode == "z" else open)(fn, "rb") as f:
        return [l for l in f.read().split(b"\n") if not l.startswith(b"##source=")]


@pytest.mark.parametrize("case", sorted(MATRIX))
def test_device_pileup_writes_the_same_files(case, inputs, tmp_path):
    vcf, depths = inputs
    flags = [depths if x is None else x for x in MATRIX[case]]
    if "--depth" not in flags and "--depths-file" not in flags:
        flags += ["--depth", "6"]
    if "-O" not in flags:
        flags += ["-O", "b"]
    mode = flags[flags.index("-O") + 1]
    res = []
    for dev in (0, 1):
        out = str(tmp_path / f"o{dev}")
        r = run(["-i", vcf, "-o", out, "--seed", "42", "-e", "0.02", "-printPileup", "1", "--device-pileup", str(dev), "--verbose", "1"] + flags)
        timing = [l for l in r.stderr.splitlines() if l.startswith("[timing]")]
        assert timing and timing[-1].rstrip().endswith("s") and ", pileup " in timing[-1]
        res.append((open(out + ".pileup.gz", "rb").read(), main_output(out, mode)))
    assert res[0][0] == res[1][0] and len(res[0][0]) > 28, case         # the compressed bytes, not only the text
    assert res[0][1] == res[1][1], case
    text = gzip.decompress(res[1][0])
    assert text.count(b"\n") > 0


@pytest.mark.parametrize("eq", [0, 1, 2])
def test_documented_error_qs_pileups_with_device_pileup(eq, tmp_path):
    out = str(tmp_path / f"error_qs{eq}")
    argv = ["-i", os.path.join(DATA, "data2.vcf"), "-o", out, "--rng-mode", "1", "--depth", "2", "--error-rate", "0.4", "--error-qs", str(eq),
            "-addFormatAD", "1", "-printPileup", "1", "--device-pileup", "1", "-s", "42", "-O", "v", "-printBasePickError", "1",
            "-printQsError", "1", "-printGlError", "1", "-printQScores", "1"]
    if eq:
        argv += ["--beta-variance", "1e-1"]
    r = run(argv)
    assert sorted(r.stdout.splitlines()) == sorted(open(os.path.join(DOC, f"details_qs{eq}.tsv")).read().splitlines())
    assert gzip.open(out + ".pileup.gz", "rt").read() == open(os.path.join(DOC, f"error_qs{eq}.pileup")).read()


def test_golden_test10_pileup_with_device_pileup(tmp_path):
    t = gu.REF_TESTS["test10"]
    assert t.get("pileup")
    out = str(tmp_path / "test10")
    run(["-i", os.path.join(DATA, t["input"]), "-o", out, "--rng-mode", "1", "--device-pileup", "1"] + t["args"].split())
    a = gzip.open(out + ".pileup.gz", "rt").read()
    b = gzip.open(os.path.join(gu.REFVCF, "reference", "test10", "test10.pileup.gz"), "rt").read()
    assert a == b
