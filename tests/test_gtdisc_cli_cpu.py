"""gtdiscordance_hip --on-device 0 (no GPU touched): the reference tool's recorded outputs byte for byte, the table modes against the
library's formatter on the model's tally, the -doGQ 1 / 2 listings and the -perSite lines against tests/gtdisc_model.py, the same
bytes from gzip, BGZF and BCF inputs, a message and exit status 1 where the tool asserts, and a clean failure of --on-device 1
without a GPU.  The library's C ABI stays what it was."""
import gzip
import os
import re
import struct
import subprocess
import zlib

import pytest

import disc_model as dm
import gtdisc_model as gm
from vcfgl_amd import _abi
from vcfgl_amd import discordance as D
from vcfgl_amd.vcfio import read_vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "misc_gtdiscordance")
VCFGL = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA3 = os.path.join(ROOT, "tests", "golden", "ref_vcf", "data", "data3.vcf")
g = lambda name: os.path.join(GOLD, "data", name)
ref = lambda name: open(os.path.join(GOLD, "reference", name)).read()


def run(tmp_path, truth, call, **kw):
    out = str(tmp_path / "out.tsv")
    rc, so, se = D.compare_files(truth, call, out, on_device=False, timeout=120, **kw)
    return rc, open(out).read() if os.path.exists(out) else None, so, se


def test_recorded_output_of_doGQ_0(tmp_path):
    rc, out, so, se = run(tmp_path, g("truth.vcf"), g("call.vcf"))
    assert rc == 0 and out == ref("test_doGq0.tsv") and so == ""
    assert gm.summary(se) == (9, 1, 8)


@pytest.mark.parametrize("call,mode", [("call3.vcf", 7), ("call3_nogq_withpl.vcf", 8), ("call3_nogq_withpl_unobservedAllele.vcf", 8)])
def test_recorded_output_of_doGQ_7_and_8(call, mode, tmp_path):
    rc, out, _, se = run(tmp_path, g("truth3.vcf"), g(call), do_gq=mode)
    assert rc == 0 and out == ref("test3_doGq7.tsv"), se[-1000:]


@pytest.mark.parametrize("mode", [3, 4, 5, 6])
def test_table_modes_are_the_librarys_formatter_on_the_models_tally(mode, tmp_path):
    truth, call = read_vcf(g("truth.vcf")), read_vcf(g("call.vcf"))
    rc, out, _, se = run(tmp_path, g("truth.vcf"), g("call.vcf"), do_gq=mode)
    assert rc == 0 and out == D.format_table(dm.tally_vcf(truth, call), truth.samples, mode), se[-1000:]
    # and the model of this program's rules gives the same table
    assert out == D.format_table(gm.compare(g("truth.vcf"), g("call.vcf"), mode).table, truth.samples, mode)


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """synthetic pairs, one per FORMAT order (no invariant records: every -doGQ mode reads them)"""
    d = tmp_path_factory.mktemp("gtdisc_pairs")
    out = []
    for k, fmt in enumerate(gm.FORMATS):
        t, c = str(d / ("t%d.vcf" % k)), str(d / ("c%d.vcf" % k))
        gm.write_pair(t, c, (1, 3, 65, 7, 2)[k], (40, 300, 12, 7, 60)[k], fmt, seed=k, first_pos=(2 ** 31 - 9 if k % 2 else 5), invariant=False,
                      odd_share=0.1 if k >= 2 else 0.0)
        out.append((fmt, t, c))
    return out


@pytest.mark.parametrize("k", range(5))
def test_listings_and_per_site_lines_are_the_models(k, pairs, tmp_path):
    fmt, t, c = pairs[k]
    for mode in ((0, 8) if fmt == "GT:PL" else (1, 2, 0, 6, 8)):
        res = gm.compare(t, c, mode, per_site=True)
        rc, out, so, se = run(tmp_path, t, c, do_gq=mode, per_site=True)
        assert res.stop is None and rc == 0, se[-1000:]
        names = gm.parse(t)[1]
        assert out == ("".join(res.listing) if mode in (1, 2) else D.format_table(res.table, names, mode))
        assert so == "".join(res.per_site) and len(so) > 0
        assert gm.summary(se) == (res.nsites1, res.nsites1 - res.nsites2, res.nsites2)


@pytest.mark.parametrize("k", range(4))
def test_listing_lines_sum_back_to_the_doGQ_6_table(k, pairs, tmp_path):
    fmt, t, c = pairs[k]
    names = gm.parse(t)[1]
    _, listing, _, _ = run(tmp_path, t, c, do_gq=2)
    _, table6, _, _ = run(tmp_path, t, c, do_gq=6)
    assert len(listing) > 0 and D.format_table(gm.table_from_listing(listing, len(names), 2), names, 6) == table6
    # -doGQ 1 is -doGQ 2 without its fourth column
    _, listing1, _, _ = run(tmp_path, t, c, do_gq=1)
    assert listing1 == "".join("\t".join(ln.split("\t")[:3] + ln.split("\t")[4:]) for ln in listing.splitlines(True))


def _bgzf(data, block=4000):
    out = b""
    for at in list(range(0, len(data), block)) + [len(data)]:               # (the last member is the empty end-of-file block)
        chunk = data[at:at + block]
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = z.compress(chunk) + z.flush()
        out += b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body
        out += struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return out


@pytest.mark.parametrize("mode", [0, 2, 8])
def test_compressed_inputs_give_the_same_bytes(mode, pairs, tmp_path):
    fmt, t, c = pairs[2]
    want = run(tmp_path, t, c, do_gq=mode, per_site=True)
    tz, cz = str(tmp_path / "t.vcf.gz"), str(tmp_path / "c.vcf.gz")
    with gzip.open(tz, "wb") as f:
        f.write(open(t, "rb").read())
    with open(cz, "wb") as f:
        f.write(_bgzf(open(c, "rb").read()))
    assert gzip.decompress(open(cz, "rb").read()) == open(c, "rb").read()
    got = run(tmp_path, tz, cz, do_gq=mode, per_site=True)
    assert got[:3] == want[:3] and want[0] == 0


@pytest.mark.skipif(not os.path.exists(VCFGL), reason="vcfgl_hip not built")
def test_a_bcf_truth_file_gives_the_table_of_its_text_form(tmp_path):
    outs = {}
    for o in ("v", "u", "b"):
        r = subprocess.run([VCFGL, "-i", DATA3, "-o", str(tmp_path / o), "-O", o, "--seed", "1", "-e", "0.01", "-d", "inf", "-printTruth", "1", "-explode", "1"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-1000:]
    truth_v = str(tmp_path / "v.truth.vcf")
    assert open(str(tmp_path / "u.truth.bcf"), "rb").read(3) == b"BCF"
    # the call file: the truth's own genotypes with a GQ, one call changed and one missing
    lines = []
    for ln in open(truth_v).read().split("\n"):
        if ln.startswith("#CHROM"):
            lines.append('##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="q">')
        if ln and not ln.startswith("#"):
            f = ln.split("\t")
            f[8] = "GT:GQ"
            f[9:] = [x.split(":")[0] + ":%d" % (1 + (7 * i + len(lines)) % 127) for i, x in enumerate(f[9:])]
            if len(lines) % 3 == 0:
                f[9] = "./.:."
            ln = "\t".join(f)
        lines.append(ln)
    call = str(tmp_path / "call.vcf")
    open(call, "w").write("\n".join(lines))
    for mode in (0, 2, 6):
        for o in ("v", "u", "b"):
            outs[o] = run(tmp_path, str(tmp_path / o) + (".truth.vcf" if o == "v" else ".truth.bcf"), call, do_gq=mode, per_site=True)
            assert outs[o][0] == 0, outs[o][3][-1000:]
        assert outs["u"][1:3] == outs["v"][1:3] == outs["b"][1:3] and len(outs["v"][1]) > 0 and len(outs["v"][2]) > 0


HEAD = ('##fileformat=VCFv4.2\n##contig=<ID=c,length=1000>\n##FORMAT=<ID=GT,Number=1,Type=String,Description="g">\n%s'
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n")
GQ_HEAD = '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="q">\n'
PL_HEAD = '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="p">\n'


def _files(tmp_path, truth_rows, call_rows, call_head=GQ_HEAD, truth_names="a\tb", call_names="a\tb"):
    t, c = str(tmp_path / "t.vcf"), str(tmp_path / "c.vcf")
    row = lambda r: "c\t%d\t.\t%s\t%s\t.\t.\t.\t%s\t%s\n" % r
    open(t, "w").write(HEAD % ("", truth_names) + "".join(row(r) for r in truth_rows))
    open(c, "w").write(HEAD % (call_head, call_names) + "".join(row(r) for r in call_rows))
    return t, c


T5 = [(5, "A", "C", "GT", "0/0\t0/1"), (7, "A", "C", "GT", "0/1\t1/1")]
STOPS = [
    ("no truth record", T5, [(5, "A", "C", "GT:GQ", "0/0:9\t0/1:9"), (6, "A", "C", "GT:GQ", "0/0:9\t0/1:9")], 6, 6, "position 6", {}),
    ("sample columns", T5, [(5, "A", "C", "GT:GQ", "0/0:9\t0/1:9"), (7, "A", "C", "GT:GQ", "0/0:9")], 6, 7, "1 sample columns", {}),
    ("haploid call", T5, [(5, "A", "C", "GT:GQ", "0/0:9\t0/1:9"), (7, "A", "C", "GT:GQ", "0/0:9\t1:9")], 6, 7, "not a diploid genotype", {}),
    ("triploid truth", [(5, "A", "C", "GT", "0/0/1\t0/1")], [(5, "A", "C", "GT:GQ", "0/0:9\t0/1:9")], 6, 5, "not a diploid genotype", {}),
    ("missing truth", [(5, "A", "C", "GT", "0/0\t./1")], [(5, "A", "C", "GT:GQ", "0/0:9\t0/1:9")], 6, 5, "true genotype is missing", {}),
    ("symbolic called allele", T5, [(5, "A", "<*>", "GT:GQ", "0/0:9\t0/1:9")], 6, 5, "ACGTacgt0123", {}),
    ("N true allele", [(5, "N", "C", "GT", "0/0\t0/1")], [(5, "A", "C", "GT:GQ", "0/0:9\t0/1:9")], 6, 5, "ACGTacgt0123", {}),
    ("index past the alleles", T5, [(5, "A", "C", "GT:GQ", "0/0:9\t0/2:9")], 6, 5, "ACGTacgt0123", {}),
    ("record without GQ", T5, [(5, "A", "C", "GT", "0/0\t0/1")], 6, 5, "has no GQ tag", {}),
    ("GQ .", T5, [(5, "A", "C", "GT:GQ", "0/0:9\t0/1:.")], 3, 5, "GQ is not a value in 1 .. 127", {}),
    ("GQ 0", T5, [(5, "A", "C", "GT:GQ", "0/0:0\t0/1:5")], 7, 5, "GQ is not a value in 1 .. 127", {}),
    ("GQ 128", T5, [(5, "A", "C", "GT:GQ", "0/0:128\t0/1:5")], 1, 5, "GQ is not a value in 1 .. 127", {}),
    ("doGQ 7 without a GQ header", T5, [(5, "A", "C", "GT", "0/0\t0/1")], 7, None, "-doGQ 7 needs a call file whose header declares the GQ tag", {"call_head": ""}),
    ("doGQ 8 without both tags", T5, [(5, "A", "C", "GT", "0/0\t0/1")], 8, None, "-doGQ 8 is only supported for genotype calling files with GQ or PL tags", {"call_head": ""}),
    ("doGQ 8: six alleles", [(5, "A", "C", "GT", "0/0\t0/1")], [(5, "A", "C,G,T,AA,CC", "GT:PL", "0/0:0\t0/1:0")], 8, 5, "6 alleles", {"call_head": PL_HEAD}),
    ("doGQ 8: no zero PL", T5, [(5, "A", "C", "GT:PL", "0/0:0,9,9\t./.:3,4,5")], 8, 5, "no PL value is 0 or missing", {"call_head": PL_HEAD}),
    ("doGQ 8: short PL", T5, [(5, "A", "C", "GT:PL", "0/0:0,9\t0/1:3,0,5")], 8, 5, "has 2 PL values", {"call_head": PL_HEAD}),
    ("sample count of the headers", T5, [(5, "A", "C", "GT:GQ", "0/0:9")], 6, None, "names 2 samples and the call file 1", {"call_names": "a"}),
]


@pytest.mark.parametrize("case", STOPS, ids=[s[0] for s in STOPS])
def test_where_the_tool_asserts_the_run_exits_1_with_a_message(case, tmp_path):
    _, truth_rows, call_rows, mode, pos, msg, kw = case
    t, c = _files(tmp_path, truth_rows, call_rows, **kw)
    rc, out, so, se = run(tmp_path, t, c, do_gq=mode)
    assert rc == 1 and "[ERROR]" in se and msg in se, se[-1000:]
    if pos is not None:
        assert ("position %d" % pos) in se
        res = gm.compare(t, c, mode)
        assert res.stop is not None and res.stop.pos == pos
    assert "Finished running" not in se


def test_a_stop_keeps_the_lines_of_the_calls_before_it(tmp_path):
    t, c = _files(tmp_path, T5, [(5, "A", "C", "GT:GQ", "0/0:9\t1/1:12"), (7, "C", "A", "GT:GQ", "1|0:33\t0/0:200")])
    rc, out, so, se = run(tmp_path, t, c, do_gq=2, per_site=True)
    assert rc == 1 and "Sample 1 at position 7" in se
    assert out == "1\t0\t0\t1\t9\n1\t1\t1\t4\t12\n2\t0\t0\t2\t33\n" and so == "5\t0\t0\t1\n5\t1\t1\t4\n7\t0\t0\t2\n"


def test_a_missing_call_is_counted_and_nothing_else(tmp_path):
    t, c = _files(tmp_path, T5, [(5, "A", "C", "GT:GQ", "./.:.\t0/1:12"), (7, "A", "C", "GT:GQ", "./1:33\t1/.:0")])
    rc, out, so, se = run(tmp_path, t, c, do_gq=0)
    assert rc == 0, se[-1000:]
    rows = [r.split("\t") for r in out.splitlines()]
    assert [r[:5] for r in rows] == [["a", "2", "2", "0", "2"], ["b", "2", "2", "1", "1"]] and rows[0][9] == "-nan"


def test_on_device_1_without_a_gpu_fails_cleanly(tmp_path):
    out = str(tmp_path / "o.tsv")
    rc, so, se = D.compare_files(g("truth.vcf"), g("call.vcf"), out, on_device=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert rc == 1 and "--on-device 1: no HIP device is available" in se and so == "" and "Finished running" not in se
    assert open(out).read() == ""


def test_help_and_bad_arguments():
    r = subprocess.run([D.GTDISC_PROGRAM, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--on-device 0|1" in r.stderr and "--batch-records" in r.stderr and "-perSite" in r.stderr
    r = subprocess.run([D.GTDISC_PROGRAM, "-t", "a", "-i", "b", "-o", "c", "-doGQ", "9"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Unknown doGq:9" in r.stderr
    r = subprocess.run([D.GTDISC_PROGRAM, "-t", "a", "-i", "b"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Output file not specified" in r.stderr


def test_the_c_abi_is_what_it_was():
    header = open(os.path.join(ROOT, "include", "vcfgl_hip.h")).read()
    assert len(_abi.EXPORTS) == len(set(_abi.EXPORTS)) == 89 == len(re.findall(r"^VGL_API\s", header, re.M)) and _abi.ABI_VERSION == 7
    assert not [e for e in _abi.EXPORTS if "gtd" in e]
    assert "exports the header's 89 entry points only" in open(os.path.join(ROOT, "README.md")).read()
    # the program's kernels are its own: the library holds none of them
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vcfgl_amd", "lib", "libvcfgl_hip.so")], capture_output=True, text=True, timeout=60).stdout
    assert "gtd" not in syms
