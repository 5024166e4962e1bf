"""setalleles_hip --on-device 0 (no GPU touched): the reference tool's two recorded outputs whole, header included; the model of the
program's rules (tests/sal_file_model.py) on generated files in the text containers; the closing stderr lines; the same for BCF, raw and BGZF, decoded
through bcf_reader and as bytes against the model's records; a message, exit status 1 and no output file wherever the run has to stop
before it writes, the records before the stop and the message where it stops at a record; the refusal across the text and BCF families; a clean failure of --on-device 1 without a GPU, and its refusal on text input."""
import os

import pytest

import sal_file_model as M
from vcfgl_amd import setalleles as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "misc_setalleles")
DATA2 = os.path.join(GOLD, "data", "data2.vcf")
EXT = {"v": ".vcf", "z": ".vcf.gz"}


def run(path, tsv, prefix, mode="v", **kw):
    return S.set_file(path, tsv, prefix, mode, on_device=False, timeout=120, **kw)


def closing(n, fn):
    return "\nProgram finished successfully!\n\t-> Processed %d sites.\n\t-> Output file: %s\n" % (n, fn)


def targets_of(tsv_path):
    return [[ln.split("\t")[0]] + ln.rstrip("\n").split("\t")[1].split(",") for ln in open(tsv_path)]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("mode", ["v", "z"])
def test_recorded_outputs_of_the_tool_whole(tmp_path, k, mode):
    tsv = os.path.join(GOLD, "data", "data2_alleles%d.tsv" % k)
    prefix = str(tmp_path / "out")
    rc, so, se = run(DATA2, tsv, prefix, mode)
    want = open(os.path.join(GOLD, "reference", "data2_alleles%d.vcf" % k), "rb").read()
    assert rc == 0 and so == "" and se == closing(10, prefix + EXT[mode])
    assert M.read_output(prefix + EXT[mode]) == want
    assert M.run_text(open(DATA2).read(), targets_of(tsv)).out.encode() == want
    assert want.split(b"\n")[:14] == open(DATA2, "rb").read().split(b"\n")[:14]             # the input's 14 header lines unchanged


def generated(tmp_path, container, **kw):
    recs = M.make_records(**kw)
    text = M.vcf_text(recs, kw["n_samples"])
    path, tsv = str(tmp_path / ("in." + container)), str(tmp_path / "a.tsv")
    M.write_file(path, text, container)
    open(tsv, "w").write(M.tsv_text(recs))
    return path, tsv, text, [r["target"] for r in recs]


@pytest.mark.parametrize("container", M.CONTAINERS)
@pytest.mark.parametrize("mode", ["v", "z"])
def test_generated_files_in_the_text_containers(tmp_path, container, mode):
    path, tsv, text, targets = generated(tmp_path, container, n_samples=9, n_records=60, seed=11, odd_share=0.2, wide_pl=True)
    want = M.run_text(text, targets)
    prefix = str(tmp_path / "out")
    rc, so, se = run(path, tsv, prefix, mode, verbose=True, threads=3)
    assert want.stop is None and 5 <= want.redone <= 25
    assert rc == 0 and se.endswith(closing(60, prefix + EXT[mode]))
    assert "records 60, redone on the host %d," % want.redone in se
    assert M.read_output(prefix + EXT[mode]).decode() == want.out


@pytest.mark.parametrize("tags", M.TAG_SETS)
@pytest.mark.parametrize("qs", [False, True])
def test_every_tag_set_with_and_without_qs(tmp_path, tags, qs):
    path, tsv, text, targets = generated(tmp_path, "vcf", n_samples=5, n_records=30, seed=3, tags=tags, qs=qs)
    want = M.run_text(text, targets)
    prefix = str(tmp_path / "out")
    rc, so, se = run(path, tsv, prefix)
    assert rc == 0 and want.stop is None and M.read_output(prefix + ".vcf").decode() == want.out


@pytest.mark.parametrize("n_old,n_new", [(o, n) for o in range(2, 6) for n in range(2, o + 1)])
def test_every_pair_of_allele_counts(tmp_path, n_old, n_new):
    path, tsv, text, targets = generated(tmp_path, "vcf", n_samples=4, n_records=20, seed=100 + 10 * n_old + n_new, n_old=n_old, n_new=n_new)
    want = M.run_text(text, targets)
    prefix = str(tmp_path / "out")
    rc, so, se = run(path, tsv, prefix)
    assert rc == 0 and want.stop is None and M.read_output(prefix + ".vcf").decode() == want.out


def test_the_default_prefix_has_the_tools_warning(tmp_path):
    tsv = os.path.join(GOLD, "data", "data2_alleles1.tsv")
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        r = S.subprocess.run([S.SETALLELES_PROGRAM, "-i", DATA2, "-a", tsv, "-O", "v", "--on-device", "0"], capture_output=True, text=True, timeout=120)
    finally:
        os.chdir(cwd)
    assert r.returncode == 0 and "Output file prefix is not specified. Setting it to 'output'." in r.stderr and r.stderr.endswith(closing(10, "output.vcf"))
    assert (tmp_path / "output.vcf").exists()


# ---- stops before any output ------------------------------------------------------------------------------------------------------------
GOOD = "A\tC,T,<*>\n"                       # a line for record 1 of data2.vcf (A / C,T,G,<*>)


@pytest.mark.parametrize("first,word", [
    ("A\n", "not REF<TAB>ALT"), ("A\tC\tG\n", "not REF<TAB>ALT"), ("A\tC,,G\n", "not REF<TAB>ALT"), ("\tC\n", "not REF<TAB>ALT"),
    ("A\t" + "C" * 253 + "\n", "256 bytes or more"), ("A\tC,G,T,<*>,N\n", "at most 4"), ("A\tC,A\n", "named twice"), ("A\tC,T,C\n", "named twice"),
])
def test_a_bad_line_of_the_alleles_file_stops_before_the_output_is_opened(tmp_path, first, word):
    rest = open(os.path.join(GOLD, "data", "data2_alleles1.tsv")).read().split("\n", 1)[1]
    tsv = str(tmp_path / "a.tsv")
    open(tsv, "w").write(first + rest)
    prefix = str(tmp_path / "out")
    rc, so, se = run(DATA2, tsv, prefix)
    assert rc == 1 and word in se and "line 1" in se and "finished" not in se and not os.path.exists(prefix + ".vcf")


def test_a_line_of_255_bytes_is_taken(tmp_path):
    names = ["A" * 120, "C" * 131]                                      # 120 + tab + 131 + newline = 253; with "G," 255
    text = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts\nc\t5\t.\t%s\t%s,G\t.\t.\t.\tGL\t-1,0,-2,-3,-4,-5\n" % tuple(names)
    path, tsv, prefix = str(tmp_path / "in.vcf"), str(tmp_path / "a.tsv"), str(tmp_path / "out")
    open(path, "w").write(text)
    line = "%s\tG,%s\n" % tuple(names)
    assert len(line) == 255
    open(tsv, "w").write(line)
    rc, so, se = run(path, tsv, prefix)
    assert rc == 0 and M.read_output(prefix + ".vcf").decode() == M.run_text(text, [[names[0], "G", names[1]]]).out


@pytest.mark.parametrize("n_lines", [9, 11])
def test_a_line_count_other_than_the_record_count(tmp_path, n_lines):
    lines = open(os.path.join(GOLD, "data", "data2_alleles1.tsv")).read().split("\n")[:10]
    tsv, prefix = str(tmp_path / "a.tsv"), str(tmp_path / "out")
    open(tsv, "w").write("".join(ln + "\n" for ln in (lines + lines)[:n_lines]))
    rc, so, se = run(DATA2, tsv, prefix)
    assert rc == 1 and "has %d lines and the record file 10 records" % n_lines in se and not os.path.exists(prefix + ".vcf")


def test_a_name_the_record_lacks_stops_with_the_position(tmp_path):
    lines = open(os.path.join(GOLD, "data", "data2_alleles1.tsv")).read().split("\n")[:10]
    lines[3] = "C\tG,AC"                                                # record 4 has C / G,A,T,<*>: compared whole, AC is none of them
    tsv, prefix = str(tmp_path / "a.tsv"), str(tmp_path / "out")
    open(tsv, "w").write("".join(ln + "\n" for ln in lines))
    rc, so, se = run(DATA2, tsv, prefix)
    want = M.run_text(open(DATA2).read(), [ln.replace("\t", ",").split(",") for ln in lines])
    assert want.stop == ("lacks", 4)
    assert rc == 1 and "names the allele AC" in se and "position 4 " in se and not os.path.exists(prefix + ".vcf")


HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\n"


def one_record(tmp_path, line, target, head=HEAD):
    path, tsv, prefix = str(tmp_path / "in.vcf"), str(tmp_path / "a.tsv"), str(tmp_path / "out")
    open(path, "w").write(head + line)
    open(tsv, "w").write("".join(t[0] + "\t" + ",".join(t[1:]) + "\n" for t in target))
    rc, so, se = run(path, tsv, prefix)
    return rc, se, prefix + ".vcf", M.run_text(head + line, target)


def test_a_record_of_six_alleles_and_a_short_qs_stop_with_the_position(tmp_path):
    rc, se, out, want = one_record(tmp_path, "c\t77\t.\tA\tC,G,T,N,<*>\t.\t.\t.\tDP\t1\t2\n", [["A", "C"]])
    assert want.stop == ("alleles", 77) and rc == 1 and "position 77 has 6 alleles" in se and not os.path.exists(out)
    rc, se, out, want = one_record(tmp_path, "c\t78\t.\tA\tC,G\t.\t.\tQS=1,0\tDP\t1\t2\n", [["A", "C"]])
    assert want.stop == ("qs", 78) and rc == 1 and "INFO/QS at position 78 has 2 values" in se and not os.path.exists(out)


# ---- stops at a record: the records before it are written -------------------------------------------------------------------------------
REC1 = "c\t10\t.\tA\tC\t.\t.\t.\tGL:PL\t0,-1,-2:0,10,20\t-3,-1,0:30,10,0\n"


@pytest.mark.parametrize("line,kind,word", [
    ("c\t11\t.\tA\tC\t.\t.\t.\tGL:PL\t0,-1,-2x:0,10,20\t-3,-1,0:30,10,0\n", "token", "Sample 0 at position 11: the GL value '-2x' is not a number"),
    ("c\t11\t.\tA\tC\t.\t.\t.\tGL:PL\t0,-1,-2:0,10,20\t-3,-1,0:30,1e1,0\n", "token", "Sample 1 at position 11: the PL value '1e1' is not an integer"),
    ("c\t11\t.\tA\tC\t.\t.\t.\tGL:PL\t0,-1,-2:0,10,20\t-3,-1,0:30,2147483648,0\n", "token", "the PL value '2147483648' is not an integer inside int32"),
    ("c\t11\t.\tA\tC\t.\t.\t.\tGL:PL\t0,-1,-2:0,10,20\n", "columns", "position 11 has 1 sample columns, the header names 2"),
    ("c\t11\t.\tA\tC\t.\t.\t.\tGL:PL\t0,-1,-2:0,10,20\t-3,-1,0:30,10,0\t.\n", "columns", "position 11 has 3 sample columns, the header names 2"),
    ("c\t11\t.\tA\tC\t.\t.\t.\tGL:PL\t0,-1,-2,-5:0,10,20\t-3,-1,0:30,10,0\n", "many", "position 11 carries more than 3 values"),
    ("c\t11\t.\tA\tC\t.\t.\t.\tGL:PL\t0,-1,-2:0,10,20\t-3,-1,0:30,10\n", "pl", "Sample 1 at position 11: PL minus its minimum does not fit int32"),
    ("c\t11\t.\tA\tC\t.\t.\t.\tGL:PL\t0,-1,-2:-2000000000,10,2000000000\t-3,-1,0:30,10,0\n", "pl", "Sample 0 at position 11: PL minus its minimum"),
])
def test_a_stop_at_a_record_leaves_the_records_before_it(tmp_path, line, kind, word):
    rc, se, out, want = one_record(tmp_path, REC1 + line + REC1.replace("\t10\t", "\t12\t"), [["C", "A"]] * 3)
    assert want.stop == (kind, 11) and want.records == 1
    assert rc == 1 and word in se and "finished" not in se
    assert open(out).read() == want.out


def test_the_rules_of_missing_and_end_of_vector(tmp_path):
    """the first NaN of a sample becomes '.', an end-of-vector among them too, and the values behind it become visible; a PL sample of
    nothing but end-of-vector becomes zeros; a NaN the arithmetic makes prints nan"""
    line = ("c\t5\t.\tA\tC,G\t.\t.\t.\tGL:PL:GP\t"
            "-1,-2:.:0,0,0,0,0,0\t"                                       # GL ragged; PL '.' with genotype 0 dropped; GP 0 / 0
            "-inf,-inf,-inf,-inf,-inf,-inf:5,4,3,2,1,0:.,1,2,3,4,5\t"        # -inf - -inf; PL whole; GP with '.' on the dropped genotype
            ".\n")                                                         # a bare '.' column
    head = HEAD.replace("s1\ts2", "s1\ts2\ts3")
    rc, se, out, want = one_record(tmp_path, line, [["G", "C"]], head)
    got = open(out).read()
    assert rc == 0 and got == want.out
    cols = got.split("\n")[-2].split("\t")
    assert cols[3:5] == ["G", "C"] and cols[9:] == [".:0,0,0:nan,nan,nan", "nan,nan,nan:0,1,3:0.454545,0.363636,0.181818", "."]


def bcf_generated(tmp_path, container, n_samples, **kw):
    recs = M.make_records(n_samples=n_samples, **kw)
    brecs = M.bcf_records(recs, n_samples, end_every=7)
    path, tsv = str(tmp_path / ("in." + container)), str(tmp_path / "a.tsv")
    M.write_bcf(path, brecs, n_samples, container)
    open(tsv, "w").write(M.tsv_text(recs))
    return path, tsv, brecs, [r["target"] for r in recs]


@pytest.mark.parametrize("container", ["bcf", "bcf.gz"])
@pytest.mark.parametrize("mode", ["u", "b"])
def test_generated_bcf_decoded_and_as_bytes(tmp_path, container, mode):
    path, tsv, brecs, targets = bcf_generated(tmp_path, container, 9, n_records=60, seed=12, wide_pl=True)
    want = M.run_bcf(brecs, targets)
    prefix = str(tmp_path / "out")
    rc, so, se = run(path, tsv, prefix, mode, threads=3)
    assert want.stop is None and rc == 0 and se == closing(60, prefix + ".bcf")
    raw = open(prefix + ".bcf", "rb").read()
    assert (raw[:2] == b"\x1f\x8b") == (mode == "b")
    body, got = M.read_bcf(prefix + ".bcf")
    assert got == want.records                                            # every field and FORMAT value, l_shared / l_indiv checked by the reader
    assert body == b"".join(M.encode_record(r, 9) for r in want.records)
    assert M.bcf_reader.Reader(prefix + ".bcf").header == M.bcf_reader.Reader(path).header
    widths = {t for r in got for k, t, per in r["fmt"] if k == "PL"}
    assert widths == {1, 2, 3}                                            # a record of each PL width
    assert any(r["rlen"] == 41 for r in got) and any(r["rlen"] == len(r["alleles"][0]) > 1 for r in got)


@pytest.mark.parametrize("tags", M.TAG_SETS)
@pytest.mark.parametrize("qs", [False, True])
def test_every_tag_set_bcf(tmp_path, tags, qs):
    path, tsv, brecs, targets = bcf_generated(tmp_path, "bcf", 5, n_records=30, seed=3, tags=tags, qs=qs)
    want = M.run_bcf(brecs, targets)
    prefix = str(tmp_path / "out")
    rc, so, se = run(path, tsv, prefix, "u")
    assert rc == 0 and want.stop is None and M.read_bcf(prefix + ".bcf")[1] == want.records


@pytest.mark.parametrize("n_old,n_new", [(o, n) for o in range(2, 6) for n in range(2, o + 1)])
def test_every_pair_of_allele_counts_bcf(tmp_path, n_old, n_new):
    path, tsv, brecs, targets = bcf_generated(tmp_path, "bcf", 4, n_records=20, seed=100 + 10 * n_old + n_new, n_old=n_old, n_new=n_new)
    want = M.run_bcf(brecs, targets)
    prefix = str(tmp_path / "out")
    rc, so, se = run(path, tsv, prefix, "u")
    body, got = M.read_bcf(prefix + ".bcf")
    assert rc == 0 and want.stop is None and got == want.records and body == b"".join(M.encode_record(r, 4) for r in want.records)


def _bcf_rec(pos, alleles, info, fmt):
    return dict(chrom="chr22", pos0=pos - 1, rlen=len(alleles[0]), qual=0x7F800001, id=".", alleles=alleles, filter=[], info=info, fmt=fmt)


def test_stops_of_a_bcf_file(tmp_path):
    f = lambda x: int(M.np.float32(x).view(M.np.uint32))
    gl3 = ("GL", 5, [[f(0), f(-1), f(-2)], [f(-3), f(-1), f(0)]])
    good = _bcf_rec(10, ["A", "C"], [], [gl3, ("PL", 1, [[0, 10, 20], [30, 10, 0]])])
    cases = [
        (_bcf_rec(11, ["A", "C", "G", "T", "N", "<*>"], [], [("DP", 1, [[1], [2]])]), ["A", "C"], "alleles", "position 11 has 6 alleles", 0),
        (_bcf_rec(11, ["A", "C"], [], [gl3]), ["A", "G"], "lacks", "names the allele G", 0),
        (_bcf_rec(11, ["A", "C"], [("QS", 5, [f(1), f(0), f(0)])], [gl3]), ["A", "C"], "qs", "INFO/QS at position 11 has 3 values", 0),
        (_bcf_rec(11, ["A", "C"], [], [("GL", 5, [[f(0), f(-1), f(-2), f(-3)]] * 2)]), ["A", "C"], "many", "FORMAT/GL at position 11 carries 4 values", 0),
        (_bcf_rec(11, ["A", "C"], [], [gl3, ("PL", 1, [[0, 10, 20], [30, 10, "END"]])]), ["C", "A"], "pl", "Sample 1 at position 11: PL minus its minimum", 1),
        (_bcf_rec(11, ["A", "C"], [], [gl3, ("PL", 3, [[-2000000000, 10, 2000000000], [30, 10, 0]])]), ["C", "A"], "pl", "Sample 0 at position 11: PL minus its minimum", 1),
    ]
    for rec, tgt, kind, word, kept in cases:
        recs, targets = [good, rec, dict(good, pos0=11)], [["C", "A"], tgt, ["C", "A"]]
        path, tsv, prefix = str(tmp_path / "in.bcf"), str(tmp_path / "a.tsv"), str(tmp_path / ("out_" + kind + str(kept)))
        M.write_bcf(path, recs, 2, "bcf")
        open(tsv, "w").write("".join(t[0] + "\t" + ",".join(t[1:]) + "\n" for t in targets))
        want = M.run_bcf(recs, targets)
        rc, so, se = run(path, tsv, prefix, "u")
        assert want.stop == (kind, 11) and rc == 1 and word in se and "finished" not in se, (kind, se)
        if kept:
            assert M.read_bcf(prefix + ".bcf")[1] == want.records and len(want.records) == 1
        else:
            assert not os.path.exists(prefix + ".bcf")
    path, tsv, prefix = str(tmp_path / "in.bcf"), str(tmp_path / "a.tsv"), str(tmp_path / "count")
    M.write_bcf(path, [good, dict(good, pos0=11)], 2, "bcf")
    open(tsv, "w").write("C\tA\n")
    rc, so, se = run(path, tsv, prefix, "u")
    assert rc == 1 and "has 1 lines and the record file 2 records" in se and not os.path.exists(prefix + ".bcf")


def test_the_rules_of_missing_and_end_of_vector_bcf(tmp_path):
    """as in text: the first NaN becomes the missing pattern, an end-of-vector too; a PL sample of nothing but end-of-vector becomes zeros"""
    f = lambda x: int(M.np.float32(x).view(M.np.uint32))
    E = M.F_END
    rec = _bcf_rec(5, ["A", "C", "G"], [("QS", 5, [f(0.5), f(0.25), f(0.125)])],
                   [("GL", 5, [[f(-1), f(-2), E, E, E, E], [f(-float("inf"))] * 6]), ("PL", 1, [[None, "END", "END", "END", "END", "END"], [5, 4, 3, 2, 1, 0]]),
                    ("GP", 5, [[0] * 6, [M.F_MISSING, f(1), f(2), f(3), f(4), f(5)]])])
    path, tsv, prefix = str(tmp_path / "in.bcf"), str(tmp_path / "a.tsv"), str(tmp_path / "out")
    M.write_bcf(path, [rec], 2, "bcf")
    open(tsv, "w").write("G\tC\n")
    rc, so, se = run(path, tsv, prefix, "u")
    got = M.read_bcf(prefix + ".bcf")[1]
    assert rc == 0 and got == M.run_bcf([rec], [["G", "C"]]).records
    Q = M.QNAN
    assert got[0]["alleles"] == ["G", "C"] and got[0]["info"] == [("QS", 5, [f(0.125), f(0.25)])]
    assert got[0]["fmt"] == [("GL", 5, [[M.F_MISSING, E, E], [Q, Q, Q]]), ("PL", 1, [[0, 0, 0], [0, 1, 3]]),
                             ("GP", 5, [[Q, Q, Q], [f(M.np.float32(5) / M.np.float32(11)), f(M.np.float32(4) / M.np.float32(11)), f(M.np.float32(2) / M.np.float32(11))]])]


def test_the_two_families_do_not_cross(tmp_path):
    tsv = os.path.join(GOLD, "data", "data2_alleles1.tsv")
    for mode in ("b", "u"):
        rc, so, se = run(DATA2, tsv, str(tmp_path / "o"), mode)
        assert rc == 1 and "Use -O v or -O z" in se and not os.path.exists(str(tmp_path / "o.bcf"))
    path, tsv, brecs, targets = bcf_generated(tmp_path, "bcf", 3, n_records=4, seed=1)
    for mode, ext in (("v", ".vcf"), ("z", ".vcf.gz")):
        rc, so, se = run(path, tsv, str(tmp_path / "o"), mode)
        assert rc == 1 and "Use -O b or -O u" in se and not os.path.exists(str(tmp_path / "o") + ext)


def test_batch_records_does_not_change_the_host_path_and_on_device_1_fails_without_a_gpu_or_on_text(tmp_path):
    path, tsv, text, targets = generated(tmp_path, "vcf", n_samples=3, n_records=10, seed=5)
    rc, so, se = run(path, tsv, str(tmp_path / "a"), batch_records=1)
    assert rc == 0 and open(str(tmp_path / "a.vcf")).read() == M.run_text(text, targets).out
    rc, so, se = S.set_file(path, tsv, str(tmp_path / "b"), "v", on_device=True, timeout=120)      # text is worked on the host: refused, no fall-back
    assert rc == 1 and "Use --on-device 0" in se and "finished" not in se and not os.path.exists(str(tmp_path / "b.vcf"))
    import torch
    if torch.cuda.is_available():
        return
    bpath, btsv, brecs, btargets = bcf_generated(tmp_path, "bcf", 3, n_records=4, seed=1)
    rc, so, se = S.set_file(bpath, btsv, str(tmp_path / "c"), "u", on_device=True, timeout=120)
    assert rc == 1 and "--on-device 1:" in se and "finished" not in se
    # a file without samples has nothing to stage and opens the GPU all the same
    M.write_bcf(bpath, [dict(r, fmt=[]) for r in brecs], 0, "bcf")
    rc, so, se = S.set_file(bpath, btsv, str(tmp_path / "d"), "u", on_device=True, timeout=120)
    assert rc == 1 and "--on-device 1:" in se and "finished" not in se
    rc, so, se = run(bpath, btsv, str(tmp_path / "d"), "u")
    assert rc == 0 and M.read_bcf(str(tmp_path / "d.bcf"))[1] == M.run_bcf([dict(r, fmt=[]) for r in brecs], btargets).records
