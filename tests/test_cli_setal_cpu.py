"""vcfgl_hip --set-alleles without a GPU: everything the flag does not support, and a bad allele file, stops the program before a device
is touched and before any file of the run exists, each with its reason."""
import os
import subprocess

import pytest

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
INPUT = os.path.join(gu.REFVCF, "data", "data3.vcf")
BASE = ["-O", "v", "--seed", "1", "-e", "0.05"]


def run(tmp_path, tsv, *flags):
    out = str(tmp_path / "out")
    r = subprocess.run([BIN, "-i", INPUT, "-o", out, "--set-alleles", tsv] + BASE + list(flags), capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and not any(f.startswith("out") for f in os.listdir(tmp_path)), r.stderr[-800:]
    return r.stderr


@pytest.mark.parametrize("flags,reason", [
    (["-d", "inf"], "--depth inf"), (["-d", "3", "-doGVCF", "1"], "-doGVCF 1"), (["-d", "3", "--rm-empty-sites", "1"], "--rm-empty-sites 1"),
    (["-d", "3", "--rm-invar-sites", "5"], "--rm-invar-sites 5"), (["-d", "3", "-addFormatAD", "1"], "the AD / ADF / ADR tags"),
    (["-d", "3", "-addInfoADF", "1"], "the AD / ADF / ADR tags"), (["-d", "3", "-addFormatADR", "1"], "the AD / ADF / ADR tags"),
    (["-d", "3", "--gt-discordance", "1"], "--gt-discordance 1"), (["-d", "3", "--fetch-gl", "AC"], "--fetch-gl AC"), (["-d", "3", "--records", "0"], "--records 0")])
def test_refusals(tmp_path, flags, reason):
    tsv = str(tmp_path / "a.tsv")
    open(tsv, "w").write("A\tC\n")
    assert "--set-alleles %s is not supported with %s" % (tsv, reason) in run(tmp_path, tsv, *flags)


@pytest.mark.parametrize("text,msg", [("A C\n", "line 1: expected REF<TAB>ALT"), ("A\tC\nA\tC,A\n", "line 2: allele A is named twice"),
                                      ("A\tC,G,T,<*>,A\n", "line 1: 5 ALT alleles; at most 4"), ("A\t<NON_REF>\n", "is spelled <*> (-doUnobserved 1), not <NON_REF>"),
                                      ("A\tN\n", "line 1: unknown allele 'N'"), ("A\tC,\n", "line 1: an empty ALT allele"), (None, "Could not open file")])
def test_bad_allele_files(tmp_path, text, msg):
    tsv = str(tmp_path / "a.tsv")
    if text is not None:
        open(tsv, "w").write(text)
    assert msg in run(tmp_path, tsv, "-d", "3")
