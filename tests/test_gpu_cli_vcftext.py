"""vcfgl_hip --device-text 1 (the sample columns of -O v / -O z records formatted on the device) writes the files --device-text 0 writes:
over a flag matrix of every FORMAT tag, both GL models, every --error-qs and --precise-gl, with and without --device-bgzf 1 and over two
contexts (--devices 0,0); and the reference's golden text outputs again with --device-text 1."""
import gzip
import os
import subprocess

import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(gu.REFVCF, "data")
ALLTAGS = ["-addGP", "1", "-addPL", "1", "-addFormatAD", "1", "-addFormatADF", "1", "-addFormatADR", "1", "-addInfoAD", "1", "-addQS", "1"]
CASES = {
    "alltags": ["-i", os.path.join(DATA, "data3.vcf"), "--depth", "6", "--error-rate", "0.01", "-explode", "1", "-printTruth", "1"] + ALLTAGS,
    "gl1": ["-i", os.path.join(DATA, "data3.vcf"), "--depth", "30", "--error-rate", "0.02", "-GL", "1", "-explode", "1", "-addPL", "1"],
    "eq1": ["-i", os.path.join(DATA, "data2.vcf"), "--depth", "3", "--error-rate", "0.05", "--error-qs", "1", "--beta-variance", "1e-5",
            "-explode", "1", "-doUnobserved", "2", "-addGP", "1", "-addFormatDP", "0"],
    "eq2precise": ["-i", os.path.join(DATA, "data3.vcf"), "--depth", "4", "--error-rate", "0.01", "--error-qs", "2", "--beta-variance", "1e-4",
                   "--precise-gl", "1", "-explode", "1", "-doUnobserved", "4", "-addI16", "1"] + ALLTAGS,
    "empty": ["-i", os.path.join(DATA, "data3.vcf"), "--depth", "0.3", "--error-rate", "0.01", "-explode", "1", "--rm-empty-sites", "1",
              "-addFormatAD", "1", "-addGL", "0"],
    "pileup": ["-i", os.path.join(DATA, "data3.vcf"), "--depth", "3", "--error-rate", "0.02", "--error-qs", "2", "--beta-variance", "1e-4",
               "-explode", "1", "-printPileup", "1", "-printQScores", "1", "-addPL", "1"],
}
MODES = {"v": [], "z": [], "z-bgzf": ["--device-bgzf", "1"], "v-devices": ["--devices", "0,0"]}


def run(out, mode, flags, extra=()):
    r = subprocess.run([BIN, "-o", out, "-O", mode, "--seed", "42", "--tile-sites", "7"] + list(extra) + flags,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def body(path):
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rt") as f:
        return [l for l in f if not l.startswith("##source=")]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("case", sorted(CASES))
def test_device_text_equals_host_text(case, mode, tmp_path):
    m = mode[0]
    ext = ".vcf" if m == "v" else ".vcf.gz"
    a, b = str(tmp_path / "host"), str(tmp_path / "dev")
    ra = run(a, m, CASES[case], MODES[mode])
    rb = run(b, m, CASES[case], MODES[mode] + ["--device-text", "1"])
    assert body(a + ext) == body(b + ext)
    assert len(body(a + ext)) > 10
    assert ra.stdout == rb.stdout                                  # per-read listings
    if os.path.exists(a + ".pileup.gz"):
        assert gzip.open(a + ".pileup.gz").read() == gzip.open(b + ".pileup.gz").read()
    if os.path.exists(a + ".truth" + ext):
        assert body(a + ".truth" + ext) == body(b + ".truth" + ext)


GOLD = [n for n in sorted(gu.REF_TESTS, key=lambda s: int(s[4:])) if n not in ("test4", "test7", "test8", "test19")]


@pytest.mark.parametrize("name", GOLD)
def test_golden_text_outputs_with_device_text(name, tmp_path):
    t = gu.REF_TESTS[name]
    argv = []
    toks = t["args"].split()
    for i in range(0, len(toks), 2):
        flag, val = toks[i], toks[i + 1]
        if flag in ("--depths-file", "--qs-bins"):
            val = os.path.join(DATA, os.path.basename(val))
        argv += [flag, val]
    assert "-doGVCF 1" not in t["args"] and "inf" not in argv
    out = str(tmp_path / name)
    r = subprocess.run([BIN, "-i", os.path.join(DATA, t["input"]), "-o", out, "--rng-mode", "1", "--device-text", "1"] + argv,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    ours = [l.rstrip("\n") for l in open(out + ".vcf") if not l.startswith("##")]
    gold = [l.rstrip("\n") for l in open(os.path.join(gu.REFVCF, "reference", name, name + ".vcf")) if not l.startswith("##")]
    assert ours == gold
