"""vcfgl_hip --fetch-gl XY: <prefix>.fetchgl.csv against what the reference's misc/fetchGl recorded (tests/golden/misc_fetchgl), against
the model of the tool (tests/fetchgl_model.py) applied to the record file the same run wrote, across every path that writes the
records, with skipped sites, and without side effects on the other files."""
import os
import subprocess

import pytest

import bcf_reader
import fetchgl_model as fm
import golden_util as gu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(gu.REFVCF, "data")
GOLD = os.path.join(gu.GOLD, "misc_fetchgl")


LAST = {}


def run(out, inp, *flags):
    r = subprocess.run([BIN, "-i", os.path.join(DATA, inp), "-o", out] + list(flags), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    LAST["stderr"] = r.stderr
    path = out + ".fetchgl.csv"
    return open(path).read() if os.path.exists(path) else None


def body(path):
    return [ln for ln in open(path) if not ln.startswith("##source=")]


def test_recorded_outputs_through_the_cli(tmp_path):
    o = lambda k: str(tmp_path / k)
    t = gu.REF_TESTS["test12"]
    got = run(o("t12"), t["input"], "--rng-mode", "1", "--fetch-gl", "CC", *t["args"].split())
    assert got == open(os.path.join(GOLD, "reference", "test12.csv")).read()
    mine = [ln for ln in open(o("t12") + ".vcf") if not ln.startswith("##")]
    assert mine == [ln for ln in open(os.path.join(GOLD, "data", "test12.vcf")) if not ln.startswith("##")]   # (the tool's own input, reproduced)
    t = gu.REF_TESTS["test10"]
    got = run(o("t10"), t["input"], "--rng-mode", "1", "--fetch-gl", "AC", *t["args"].split())
    want = fm.file_lines(open(os.path.join(gu.REFVCF, "reference", "test10", "test10.vcf")).read(), "AC")
    assert got == want and len(got.splitlines()) == 10
    assert got.startswith(open(os.path.join(GOLD, "reference", "test10_AC_head.csv")).read())


CASES = [("data3.vcf", ["-explode", "1", "-d", "3"], "AC"),
         ("data5_acgt_multiallelic.vcf", ["--source", "1", "-d", "2"], "GT"),
         ("data3.vcf", ["-explode", "1", "-d", "2", "-doUnobserved", "2"], "A<")]


def bcf_lines(path, gt):
    """%f of the floats a BCF holds, by the tool's rules"""
    out = []
    for rec in bcf_reader.Reader(path).records():
        g = fm.genotype_index([a[0] for a in rec["alleles"]], gt)
        if g is None:
            continue
        per = next(p for k, t, p in rec["fmt"] if k == "GL")
        out.append("%d," % (rec["pos0"] + 1) + ",".join(fm.fmt_value_bits(v[g], fm.FLOAT) if g < len(v) else "END" for v in per) + "\n")
    return "".join(out)


@pytest.mark.parametrize("inp,src,gt", CASES, ids=["binary", "acgt_multiallelic", "unobserved"])
def test_csv_equals_the_model_of_the_runs_own_file_on_every_path(inp, src, gt, tmp_path):
    o = lambda k: str(tmp_path / k)
    base = ["--seed", "42", "-e", "0.05", "--tile-sites", "7", "-addPL", "1", "--fetch-gl", gt] + src
    csv = run(o("v"), inp, "-O", "v", *base)
    assert csv == fm.file_lines(open(o("v") + ".vcf").read(), gt) and csv.count("\n") > 0
    ucsv = run(o("u"), inp, "-O", "u", *base)
    assert ucsv == bcf_lines(o("u") + ".bcf", gt) and ucsv.count("\n") == csv.count("\n")
    assert run(o("u1"), inp, "-O", "u", "--fetch-gl-value", "1", *base) == csv
    assert run(o("v2"), inp, "-O", "v", "--fetch-gl-value", "2", *base) == ucsv
    # the same CSV whatever writes the records
    assert run(o("txt"), inp, "-O", "v", "--device-text", "1", *base) == csv
    assert run(o("bcf"), inp, "-O", "b", "--device-bcf", "1", "--device-stream", "1", "--fetch-gl-value", "1", *base) == csv
    assert run(o("dev2"), inp, "-O", "v", "--devices", "0,0", *base) == csv
    assert run(o("pile"), inp, "-O", "v", "-printPileup", "1", "--device-pileup", "1", *base) == csv
    assert run(o("disc"), inp, "-O", "v", "--gt-discordance", "1", *base) == csv
    assert run(o("norec"), inp, "--records", "0", "--fetch-gl-value", "1", *base) == csv
    assert sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("norec")) == ["norec.arg", "norec.fetchgl.csv"]
    assert run(o("norec2"), inp, "--records", "0", "--gt-discordance", "1", *base) == ucsv        # (-O's default is b: the simulated floats)
    # without the flag: no CSV, and the same records
    assert run(o("off"), inp, "-O", "v", *[x for x in base if x not in ("--fetch-gl", gt)]) is None
    assert body(o("off") + ".vcf") == body(o("v") + ".vcf") == body(o("txt") + ".vcf") == body(o("disc") + ".vcf")
    assert open(o("disc") + ".discordance.tsv").read() == open(o("norec2") + ".discordance.tsv").read()


def test_with_skipped_sites_and_the_serial_draw_order(tmp_path):
    """--rm-empty-sites 1 --rm-invar-sites 4 at depth 0.7: the CSV lacks exactly the sites the record file lacks"""
    import re
    o = lambda k: str(tmp_path / k)
    base = ["--seed", "42", "-e", "0.05", "--tile-sites", "7", "-explode", "1", "-d", "0.7", "--rm-empty-sites", "1", "--rm-invar-sites", "4",
            "-O", "v", "--verbose", "1"]
    lines = 0
    for mode in ("0", "1"):
        for gt in ("AA", "CC", "<<"):
            k = "rm%s%s" % (mode, gt.replace("<", "x"))
            csv = run(o(k), "data3.vcf", "--rng-mode", mode, "--fetch-gl", gt, *base)
            recs = [ln.split("\t")[1] for ln in open(o(k) + ".vcf") if not ln.startswith("#")]
            assert csv == fm.file_lines(open(o(k) + ".vcf").read(), gt)
            pos = [ln.split(",")[0] for ln in csv.splitlines()]
            assert set(pos) <= set(recs)
            m = re.search(r"\[fetch-gl\].* (\d+) lines written, (\d+) sites without the genotype", LAST["stderr"])
            assert m and int(m.group(1)) == len(pos) and int(m.group(1)) + int(m.group(2)) == len(recs)
            assert int(re.search(r"Number of sites skipped: (\d+)", LAST["stderr"]).group(1)) > 0
            assert "Fetched genotype likelihoods file" in open(o(k) + ".arg").read()
            lines += len(pos)
    assert lines > 0
