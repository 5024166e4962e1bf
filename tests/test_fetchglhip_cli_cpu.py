"""fetchgl_hip --on-device 0 (no GPU touched): the reference tool's recorded outputs byte for byte, the model of the program's rules
(tests/fgl_file_model.py) on generated files in all four containers for every value index 0 .. 14, -o and --messages 0, a message and
exit status 1 with the position wherever the run has to stop, the same bytes whatever --batch-records says, and a clean failure of
--on-device 1 without a GPU.  The library's C ABI stays what it was."""
import os
import re
import subprocess

import pytest

import fetchgl_model as fm
import fgl_file_model as gm
from vcfgl_amd import _abi
from vcfgl_amd import fetchgl as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TEST12 = os.path.join(GOLD, "misc_fetchgl", "data", "test12.vcf")
TEST10 = os.path.join(GOLD, "ref_vcf", "reference", "test10", "test10.vcf")
ref = lambda name: open(os.path.join(GOLD, "misc_fetchgl", "reference", name)).read()

# the stderr lines the reference's misc/README.md lists for -i test10.vcf -gt AC
README_STDERR = "".join("Requested genotype's first allele corresponds to allele %d and second allele corresponds to allele %d at position %d.\n" % (a, b, p)
                        for p, (a, b) in enumerate([(0, 1)] * 3 + [(1, 0)] * 3 + [(0, 1)] * 4, 1))


def run(path, gt, **kw):
    return F.fetch_file(path, gt, on_device=False, timeout=120, **kw)


def test_recorded_output_of_the_tools_own_test():
    rc, so, se = run(TEST12, "CC")
    assert rc == 0 and so == ref("test12.csv")
    assert so == fm.file_lines(open(TEST12).read(), "CC") == "".join(gm.run_file(TEST12, "CC").stdout)
    assert se == "".join(gm.run_file(TEST12, "CC").messages)


def test_the_listing_of_the_tools_readme():
    rc, so, se = run(TEST10, "AC")
    assert rc == 0
    head = ref("test10_AC_head.csv")
    assert head.count("\n") == 8 and so.startswith(head)
    assert README_STDERR.count("\n") == 10 and se.startswith(README_STDERR)
    res = gm.run_file(TEST10, "AC")
    assert so == "".join(res.stdout) and se == "".join(res.messages)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """one set of records with the fixed alleles A,C,G,T,<*> (every g of 0 .. 14 has a genotype) and one with drawn alleles, each in
    the four containers; a tenth of the records holds tokens outside the device grammar"""
    d = tmp_path_factory.mktemp("fgl_files")
    out = {}
    for name, fixed, n, n_rec, first in (("fixed", True, 5, 40, 95), ("drawn", False, 3, 120, 2 ** 31 - 119)):
        recs = gm.make_records(n, n_rec, seed=11 if fixed else 12, first_pos=first, odd_share=0.1, fixed_alleles=fixed)
        for c in gm.CONTAINERS:
            out[name, c] = gm.write_file(str(d / ("%s.%s" % (name, c))), recs, n, c)
    return out


def same_as_model(path, gt, **kw):
    res = gm.run_file(path, gt)
    rc, so, se = run(path, gt, verbose=True, **kw)
    assert rc == res.returncode == 0, se[-1000:]
    assert so == "".join(res.stdout)
    lines = se.splitlines(True)
    assert "".join(lines[:-1]) == "".join(res.messages)
    m = re.match(r"\[fetchgl\] on-device 0: records (\d+), with a CSV line (\d+), redone on the host (\d+),", lines[-1])
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (len(res.messages), res.lines, res.redone)
    return res


@pytest.mark.parametrize("container", gm.CONTAINERS)
def test_every_value_index_equals_the_model(container, files):
    seen = set()
    for g, gt in enumerate(gm.GENOTYPES):
        assert fm.genotype_index([a[0] for a in gm.FIXED_ALLELES], gt) == g
        res = same_as_model(files["fixed", container], gt)
        assert res.lines == 40
        seen |= {v for ln in res.stdout for v in ln.rstrip("\n").split(",")[1:] if not v[-1].isdigit()}
        if container != "bcf":
            assert 1 <= res.redone <= 12                               # the odd records are redone, and only they
    assert seen >= {"MISSING", "END", "inf", "-inf", "nan"}


@pytest.mark.parametrize("container", gm.CONTAINERS)
def test_drawn_alleles_equal_the_model(container, files):
    lines = 0
    for gt in ("AC", "CA", "A<", "<<", "GG", "TC", "Na", "ZZ", "A*"):
        res = same_as_model(files["drawn", container], gt)
        lines += res.lines
        assert any("not found" in m for m in res.messages)
    assert lines > 50
    assert same_as_model(files["drawn", container], "ZZ").lines == 0


def test_the_containers_give_the_same_bytes(files):
    for name, gt in (("fixed", "CG"), ("drawn", "GA")):
        outs = [run(files[name, c], gt) for c in gm.CONTAINERS]
        assert outs[0][0] == 0 and len(outs[0][1]) > 0
        assert outs[0] == outs[1] == outs[2]
        assert outs[3][2] == outs[0][2]                                # BCF: the same messages; the values are the stored floats
        assert outs[3][1] == "".join(gm.run_file(files[name, "bcf"], gt).stdout)


def test_output_file_and_messages_off(files, tmp_path):
    path = files["fixed", "vcf"]
    rc, so, se = run(path, "AT")
    out = str(tmp_path / "o.csv")
    rc2, so2, se2 = run(path, "AT", out=out, messages=False)
    assert rc == rc2 == 0 and so2 == "" and se2 == "" and open(out).read() == so and len(so) > 0 and se.count("\n") == 40


@pytest.mark.parametrize("batch", [1, 7, 4096])
def test_output_does_not_depend_on_batch_records(batch, files):
    for c in ("vcf", "bcf"):
        assert run(files["drawn", c], "AC", batch_records=batch) == run(files["drawn", c], "AC")


HEAD = ('##fileformat=VCFv4.2\n##contig=<ID=c,length=1000>\n##FORMAT=<ID=GT,Number=1,Type=String,Description="g">\n%s'
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\n")
GL_HEAD = '##FORMAT=<ID=GL,Number=G,Type=Float,Description="l">\n'
ROW = "c\t%d\t.\t%s\t%s\t.\t.\t.\t%s\t%s\n"
OK5 = (5, "A", "C", "GT:GL", "0/0:-1,-2,-3\t0/1:-4,-5,-6")
STOPS = [
    ("header without GL", "", [OK5], "AC", 5, "gl", "Could not read GL tag"),
    ("record without GL", GL_HEAD, [OK5, (7, "A", "C", "GT", "0/0\t0/1")], "AC", 7, "gl", "Could not read GL tag"),
    ("record without GL and without the genotype", GL_HEAD, [OK5, (7, "A", "G", "GT", "0/0\t0/1")], "AC", 7, "gl", "Could not read GL tag"),
    ("value index past every sample's values", GL_HEAD, [OK5, (7, "A", "C", "GT:GL", "0/0:-1,-2\t0/1:-4")], "CC", 7, "range", "at most 2 values"),
    ("value index past a '.' field", GL_HEAD, [OK5, (7, "A", "C", "GT:GL", "0/0:.\t0/1")], "AC", 7, "range", "at most 1 values"),
    ("a sample column missing", GL_HEAD, [OK5, (7, "A", "C", "GT:GL", "0/0:-1,-2,-3")], "AC", 7, "columns", "1 sample columns"),
    ("a sample column too many", GL_HEAD, [OK5, (7, "A", "C", "GT:GL", "0/0:-1,-2,-3\t0/1:-4,-5,-6\t0/1:-4,-5,-6")], "AC", 7, "columns", "3 sample columns"),
    ("a token strtod stops in", GL_HEAD, [OK5, (7, "A", "C", "GT:GL", "0/0:-1,-2x,-3\t0/1:-4,-5,-6")], "AC", 7, "token", "'-2x' is not a number"),
    ("an empty token", GL_HEAD, [OK5, (7, "A", "C", "GT:GL", "0/0:-1,,-3\t0/1:-4,-5,-6")], "AC", 7, "token", "'' is not a number"),
    ("an exponent without digits", GL_HEAD, [OK5, (7, "A", "C", "GT:GL", "0/0:-1,-2,-3\t0/1:-4,1e,-6")], "AC", 7, "token", "'1e' is not a number"),
]


@pytest.mark.parametrize("case", STOPS, ids=[s[0] for s in STOPS])
def test_where_the_run_has_to_stop_it_exits_1_with_the_position(case, tmp_path):
    _, head, rows, gt, pos, kind, msg = case
    path = str(tmp_path / "in.vcf")
    open(path, "w").write(HEAD % head + "".join(ROW % r for r in rows))
    res = gm.run_file(path, gt)
    assert res.stop == (kind, pos)
    rc, so, se = run(path, gt)
    assert rc == 1 and "[ERROR]" in se and msg in se and ("position %d" % pos) in se, se[-1000:]
    assert so == "".join(res.stdout) and se.startswith("".join(res.messages))     # the lines and messages before it are written
    assert se[len("".join(res.messages)):].lstrip("\n").startswith("*******")


def test_an_unpicked_token_is_not_judged(tmp_path):
    """only the value the genotype picks is read: our decision (fgl_core.h) -- the tool's reader would have parsed the others too"""
    path = str(tmp_path / "in.vcf")
    open(path, "w").write(HEAD % GL_HEAD + ROW % (7, "A", "C", "GT:GL", "0/0:-1,-2x,-3\t0/1:-4,-5,-6"))
    rc, so, se = run(path, "AA")
    assert rc == 0 and so == "7,-1.000000,-4.000000\n"


def test_bcf_stops(tmp_path):
    recs = gm.make_records(3, 6, seed=3, first_pos=10, fixed_alleles=True, fmt="GT:GL")
    path = gm.write_file(str(tmp_path / "int.bcf"), recs, 3, "bcf", gl_type="Integer")       # GL defined as anything but Float
    rc, so, se = run(path, "AC")
    assert rc == 1 and "Could not read GL tag at position 10" in se and so == "" and gm.run_file(path, "AC").stop == ("gl", 10)
    for c in recs[3]["cols"]:                                                               # a record whose vectors are shorter than g
        if c["GL"]:
            c["GL"] = ",".join(c["GL"].split(",")[:2])
    path = gm.write_file(str(tmp_path / "short.bcf"), recs, 3, "bcf")
    res = gm.run_file(path, "CC")
    rc, so, se = run(path, "CC")
    assert res.stop == ("range", 13) and rc == 1 and "position 13" in se and "at most 2 values" in se
    assert so == "".join(res.stdout) and so.count("\n") == 3 and se.startswith("".join(res.messages))


def test_bad_arguments():
    r = subprocess.run([F.FETCHGL_PROGRAM, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--on-device 0|1" in r.stderr and "--batch-records" in r.stderr and "--messages" in r.stderr
    for gt in ("A", "ACG"):
        rc, so, se = run(TEST12, gt)
        assert rc == 1 and "exactly two characters" in se and so == ""
    r = subprocess.run([F.FETCHGL_PROGRAM, "-i", TEST12], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Genotype to fetch not specified" in r.stderr
    r = subprocess.run([F.FETCHGL_PROGRAM, "-gt", "AC"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Input file not specified" in r.stderr


def test_on_device_1_without_a_gpu_fails_cleanly():
    rc, so, se = F.fetch_file(TEST12, "CC", on_device=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert rc == 1 and "--on-device 1: no HIP device is available" in se and so == "" and "Requested genotype" not in se


def test_the_c_abi_is_what_it_was():
    header = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    assert len(_abi.EXPORTS) == len(set(_abi.EXPORTS)) == 89 == len(re.findall(r"^VGL_API\s", header, re.M)) and _abi.ABI_VERSION == 7
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vcfgl_amd", "lib", "libvcfgl_hip.so")], capture_output=True, text=True, timeout=60).stdout
    assert "fgl" not in syms
