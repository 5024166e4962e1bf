"""fetchgl_hip --resident 1 (misc/resident_file.hip: a BGZF file of VCF text is inflated into GPU memory and stays there; the GPU
finds the lines, their heads alone come down, the sample columns are parsed where the inflater wrote them): every byte the run writes
-- the CSV on stdout or in the -o file, the messages, the error a run stops with -- is what --on-device 0 writes, on generated files
whose shapes put workgroup and batch boundaries everywhere, on the golden inputs as BGZF, on texts built around RF_CHUNK (read from
the program's own line, not copied), on records the device hands back, and on the files that cannot be resident, where the run goes
on as --resident 0 and says why.  rf_check holds the device's split against scan_text / nine_columns on zlib's bytes.

Every GPU process runs under a timeout; after a process that faulted, aborted or ran out of time nothing more is started."""
import os

import numpy as np
import pytest

import fgl_file_model as gm
import miscread_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TEST12 = os.path.join(GOLD, "misc_fetchgl", "data", "test12.vcf")
TEST10 = os.path.join(GOLD, "ref_vcf", "reference", "test10", "test10.vcf")


def _resident(path, gt, **kw):
    return U.fetch(path, gt, on_device=True, device_inflate=True, resident=True, **kw)


def _same(tmp_path, path, gt, with_file=True, host=None, **kw):
    """--resident 1 against --on-device 0 on one file: return code, stdout, the -o file and stderr (messages and the error)"""
    rh = host or U.fetch(path, gt, on_device=False, **kw)
    rd = _resident(path, gt, **kw)
    assert rd[0] == rh[0], (rd[2][-2000:], rh[2][-2000:])
    assert rd[1] == rh[1]
    assert U.plain(rd[2]) == U.plain(rh[2])
    if with_file:
        od = str(tmp_path / "dev.csv")
        fd = _resident(path, gt, out=od, **kw)
        assert fd[0] == rh[0] and fd[1] == "" and open(od, "rb").read() == rh[1].encode() and U.plain(fd[2]) == U.plain(rh[2])
    return rh, rd


def _is_resident(stderr, lines=None):
    res = U.resident_line(stderr)
    assert res["resident"] == 1 and res["why"] is None and res["members"] > 0 and res["up"] > 0 and res["head_bytes"] >= res["lines"], res
    assert not U.inflate_lines(stderr)                                 # no part of the file came down whole
    if lines is not None:
        assert res["lines"] == lines
    return res


def _bgzf_file(tmp_path, name, text, block=60000):
    return U.write(tmp_path / name, gm.bgzf(text, block=block))


SHAPES = [(n, r) for n in (1, 63, 64, 65, 257) for r in (1, 7, 300)]


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_generated_files(k, tmp_path):
    n, n_records = SHAPES[k]
    first = 2 ** 31 - n_records + 1 if k % 2 else 8
    recs = gm.make_records(n, n_records, seed=3000 + k, first_pos=first, fixed_alleles=True)
    text = gm.vcf_text(recs, n).encode()
    path = _bgzf_file(tmp_path, "in.vcf.gz", text, block=(60000, 4096, 9973)[k % 3])
    header_lines = text.count(b"\n") - n_records
    for j, batch in enumerate((1, 7, 4096)):
        gt = gm.GENOTYPES[(3 * k + j) % 15]
        rh, rd = _same(tmp_path, path, gt, with_file=(j == 2), batch_records=batch)
        assert rh[0] == 0, rh[2][-2000:]
        _is_resident(rd[2], lines=n_records + header_lines)
        records, with_line, redone, up, down = U.fetch_counts(rd[2])
        assert (records, with_line, redone) == (n_records, n_records, 0) and down > 0
        assert up == n_records * 32                                    # descriptors alone go up: no text is staged
    if n_records == 300:                                               # drawn alleles: records without the genotype between those with it
        recs = gm.make_records(n, n_records, seed=4000 + k, first_pos=first)
        path = _bgzf_file(tmp_path, "drawn.vcf.gz", gm.vcf_text(recs, n).encode())
        rh, rd = _same(tmp_path, path, "AC", batch_records=7)
        records, with_line, redone, _, _ = U.fetch_counts(rd[2])
        assert rh[0] == 0 and records == 300 and 0 < with_line < 300 and redone == 0
        _is_resident(rd[2])


def test_golden_inputs_as_bgzf(tmp_path):
    for name, src, gts in (("t12.vcf.gz", TEST12, ("CC", "AC", "GT")), ("t10.vcf.gz", TEST10, ("AC", "TT"))):
        text = open(src, "rb").read()
        path = _bgzf_file(tmp_path, name, text, block=5000)
        lines = 0
        for gt in gts:
            rh, rd = _same(tmp_path, path, gt, host=U.fetch(src, gt, on_device=False))
            assert rh[0] == 0, rh[2][-2000:]
            _is_resident(rd[2], lines=text.count(b"\n") + (0 if text.endswith(b"\n") else 1))
            records, with_line, redone, _, _ = U.fetch_counts(rd[2])
            assert redone == 0
            lines += with_line
        assert lines > 0
    assert _resident(str(tmp_path / "t12.vcf.gz"), "CC")[1] == open(os.path.join(GOLD, "misc_fetchgl", "reference", "test12.csv")).read()


def test_more_members_than_one_inflate_call(tmp_path):
    """the inflater is called for 4096 members at a time: members of 13 bytes make a second call, and lines that lie across many members"""
    recs = gm.make_records(65, 7, seed=77, first_pos=95, fixed_alleles=True)
    text = gm.vcf_text(recs, 65).encode()
    path = _bgzf_file(tmp_path, "small_members.vcf.gz", text, block=13)
    rh, rd = _same(tmp_path, path, "CG", with_file=False)
    res = _is_resident(rd[2], lines=text.count(b"\n"))
    assert rh[0] == 0 and res["members"] == -(-len(text) // 13) + 1 > 4096 and U.fetch_counts(rd[2])[:3] == (7, 7, 0)


@pytest.fixture(scope="module")
def chunk(tmp_path_factory):
    """RF_CHUNK as the programs print it"""
    d = tmp_path_factory.mktemp("rf_chunk")
    path = U.write(d / "tiny.vcf.gz", gm.bgzf(U.text_of_length(2, 600)))
    rc, so, se = U.rf_check(path)
    assert rc == 0 and "differences 0" in so, (so, se)
    c = int(so.split("RF_CHUNK ")[1].split(",")[0])
    assert U.resident_line(_resident(path, "AC")[2])["chunk"] == c and c >= 64
    return c


def boundary_texts(C, n=3):
    t = {}
    t["newline_last_of_a_chunk"] = U.text_with(n, 4, "newline", 2 * C - 1)
    t["newline_first_of_a_chunk"] = U.text_with(n, 4, "newline", 2 * C)
    t["tab9_last_of_a_chunk"] = U.text_with(n, 4, "tab9", 2 * C - 1)
    t["tab9_first_of_a_chunk"] = U.text_with(n, 4, "tab9", 2 * C)
    t["line_over_three_chunks"] = U.text_with(n, 2, "newline", 4 * C + 17)
    t["line_begins_at_a_chunk"] = U.text_with(n, 4, "begin", 3 * C)
    t["total_two_chunks"] = U.text_of_length(n, 2 * C)
    t["total_chunk_minus_1"] = U.text_of_length(n, C - 1) if C > 700 else U.text_of_length(n, 8 * C - 1)
    t["total_chunk_plus_1"] = U.text_of_length(n, C + 1) if C > 700 else U.text_of_length(n, 8 * C + 1)
    t["no_trailing_newline"] = U.text_of_length(n, C + 300, newline=False)
    body = ("\n".join(U.HEAD + [U.names_line(n)]) + "\n").encode()
    recs = [U.record(10 + i, n).encode() for i in range(4)]
    t["empty_lines"] = b"\n\n" + body + b"\n" + recs[0] + b"\n\n\n" + recs[1] + b"\n" + recs[2] + b"\n\n\n"
    t["header_line_after_the_records"] = body + recs[0] + b"\n" + recs[1] + b"\n##late=1\n" + recs[2] + b"\n"
    t["header_only"] = body
    t["eight_columns"] = body + recs[0] + b"\n" + U.record(11, n, columns=8).encode() + b"\n" + recs[2] + b"\n"
    return t


BOUNDARIES = sorted(boundary_texts(4096))


@pytest.mark.parametrize("name", BOUNDARIES)
def test_boundaries(name, chunk, tmp_path):
    text = boundary_texts(chunk)[name]
    path = _bgzf_file(tmp_path, "b.vcf.gz", text, block=1500)
    rh, rd = _same(tmp_path, path, "AC", with_file=False, batch_records=2)
    n_lines = text.count(b"\n") + (0 if text.endswith(b"\n") else 1)
    _is_resident(rd[2], lines=n_lines)
    if name == "eight_columns":
        assert rh[0] == 1 and "Record 2 has fewer than 10 columns" in rd[2] and rd[1].count("\n") == 1
    elif name == "header_only":
        assert rh[0] == 0 and rd[1] == ""
    else:
        assert rh[0] == 0 and rd[1].count("\n") == sum(1 for ln in text.split(b"\n") if ln and ln[:1] != b"#"), rh[2][-1500:]
    rc, so, se = U.rf_check(path)
    assert rc == 0 and "over 0, differences 0" in so and ("lines %d," % n_lines) in so and ("total %d," % len(text)) in so, (so, se)


def test_random_fixed_columns_through_rf_check(chunk, tmp_path):
    rng = np.random.default_rng(11)
    printable = [chr(c) for c in range(32, 127)]
    col = lambda: "".join(rng.choice(printable, size=int(rng.integers(0, 51))))
    lines = U.HEAD + [U.names_line(4)]
    for i in range(200):
        lines.append("\t".join(["chr22", str(100 + i), col(), "A", "C", col(), col(), col(), "GL"] + ["-1,-2,-3"] * 4))
    text = ("\n".join(lines) + "\n").encode()
    rc, so, se = U.rf_check(_bgzf_file(tmp_path, "r.vcf.gz", text, block=777))
    assert rc == 0 and "records 200," in so and "over 0, differences 0" in so and ("lines %d," % len(lines)) in so, (so, se)


def test_handed_back_records(tmp_path):
    recs = gm.make_records(65, 300, seed=5, fixed_alleles=True, odd_share=0.1)
    text = gm.vcf_text(recs, 65).encode()
    plain_path = U.write(tmp_path / "odd.vcf", text)
    want = gm.run_file(plain_path, "CG")
    path = _bgzf_file(tmp_path, "odd.vcf.gz", text)
    rh, rd = _same(tmp_path, path, "CG", batch_records=64)
    assert rh[0] == 0 and rd[1] == "".join(want.stdout)
    _is_resident(rd[2])
    records, with_line, redone, _, _ = U.fetch_counts(rd[2])
    assert (records, with_line) == (300, 300) and redone == want.redone == U.fetch_counts(rh[2])[2]
    assert 10 <= redone <= 60                                          # about one record in ten (the generator's share, 300 draws)
    recs = gm.make_records(65, 300, seed=5, fixed_alleles=True, odd_share=0.0)
    path = _bgzf_file(tmp_path, "plain.vcf.gz", gm.vcf_text(recs, 65).encode())
    rh, rd = _same(tmp_path, path, "CG", with_file=False, batch_records=64)
    assert U.fetch_counts(rd[2])[:3] == (300, 300, 0)


@pytest.mark.parametrize("place", [0, 3, 6])
def test_a_record_out_of_range_stops_the_run_where_the_host_stops(place, tmp_path):
    """batches of 7 records: record 14 + place is the first, a middle or the last of its batch"""
    recs = gm.make_records(65, 30, seed=9, first_pos=100, fixed_alleles=True, fmt="GT:GL")
    at = 14 + place
    for c in recs[at]["cols"]:
        if c["GL"]:
            c["GL"] = ",".join(c["GL"].split(",")[:6])
    text = gm.vcf_text(recs, 65).encode()
    want = gm.run_file(U.write(tmp_path / "range.vcf", text), "GT")    # g = 8
    assert want.stop == ("range", 100 + at)
    path = _bgzf_file(tmp_path, "range.vcf.gz", text, block=7000)
    rh, rd = _same(tmp_path, path, "GT", batch_records=7)
    assert rd[0] == 1 and rd[1] == "".join(want.stdout) and rd[1].count("\n") == at
    assert "position %d" % (100 + at) in rd[2] and "at most 6 values" in rd[2] and U.plain(rd[2]).startswith("".join(want.messages))
    _is_resident(rd[2])
    recs[at]["cols"].pop()                                             # a column too few there instead
    path = _bgzf_file(tmp_path, "short.vcf.gz", gm.vcf_text(recs, 65).encode(), block=7000)
    rh, rd = _same(tmp_path, path, "AC", batch_records=7)
    assert rd[0] == 1 and rd[1].count("\n") == at and "64 sample columns" in rd[2]


def _goes_on_as_resident_0(tmp_path, path, gt, why, **kw):
    rh = U.fetch(path, gt, on_device=False)
    rd = _resident(path, gt, **kw)
    assert rd[0] == rh[0] == 0 and rd[1] == rh[1] and len(rd[1]) > 0 and U.plain(rd[2]) == U.plain(rh[2]), (rd[2][-1500:], rh[2][-1500:])
    res = U.resident_line(rd[2])
    assert res["resident"] == 0 and why in res["why"], res
    (ln,) = U.inflate_lines(rd[2])                                     # the bytes came through the device inflater all the same
    assert not ln["host"] and ln["members"] > 0 and ln["down"] > 0
    od = str(tmp_path / "dev.csv")
    fd = _resident(path, gt, out=od, **kw)
    assert fd[0] == 0 and open(od, "rb").read() == rh[1].encode()
    return res


def test_goes_on_as_resident_0(tmp_path):
    recs = gm.make_records(5, 20, seed=21, fixed_alleles=True)
    text = gm.vcf_text(recs, 5).encode()
    path = _bgzf_file(tmp_path, "small.vcf.gz", text)
    _goes_on_as_resident_0(tmp_path, path, "AC", "--resident-max-bytes", resident_max_bytes=1000)
    _is_resident(_resident(path, "AC", resident_max_bytes=len(text) + os.path.getsize(path))[2])      # exactly enough
    bcf = U.write(tmp_path / "small.bcf", gm.bgzf(gm.bcf_bytes(recs, 5)))
    _goes_on_as_resident_0(tmp_path, bcf, "AC", "BCF")
    # a record whose first column alone is longer than the walk for the ninth tab
    lines = U.HEAD + [U.names_line(1), U.record(10, 1), "c" * (1100 * 1024) + U.record(11, 1)[5:], U.record(12, 1)]
    long_path = _bgzf_file(tmp_path, "long.vcf.gz", ("\n".join(lines) + "\n").encode())
    res = _goes_on_as_resident_0(tmp_path, long_path, "AC", "ninth tab")
    assert res["lines"] == len(lines)
    rc, so, se = U.rf_check(long_path, 64)
    assert rc == 0 and "over 1" in so, (so, se)
    rc, so, se = U.rf_check(long_path, 2 << 20)                         # with a longer walk the same file splits
    assert rc == 0 and "over 0, differences 0" in so, (so, se)
