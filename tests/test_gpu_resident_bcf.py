"""fetchgl_hip --resident-bcf 1 (misc/resident_file.hip, misc/rb_core.h: a BGZF file of BCF is inflated into GPU memory and stays there;
the GPU follows the records' lengths and walks their FORMAT fields, the heads alone come down, the GL vectors are read where the
inflater wrote them, at whatever byte they begin): every byte the run writes -- the CSV on stdout or in the -o file, the messages, the
error a run stops with -- is what --on-device 0 writes, on generated files over sample counts, record counts, batch sizes and member
sizes, on drawn alleles that put the GL blocks at all four residues mod 4, on members of 13 bytes, on runs that stop, on a file the
simulator wrote, and on the files that cannot be resident, where the run goes on as --resident 0 and says why.  rb_check holds the
device's walk against bcf_scan_record / bcf_format_fields on zlib's bytes, at 1, 2 and 7 records a chain launch.

Every GPU process runs under a timeout; after a process that faulted, aborted or ran out of time nothing more is started."""
import gzip
import os
import struct
import subprocess

import pytest

import fgl_file_model as gm
import miscread_util as U
import residentbcf_util as R

pytestmark = pytest.mark.gpu

DATA = os.path.join(U.ROOT, "tests", "golden", "ref_vcf", "data")
VCFGL = os.path.join(U.ROOT, "vcfgl_amd", "bin", "vcfgl_hip")


def _resident(path, gt, **kw):
    return U.fetch(path, gt, on_device=True, device_inflate=True, resident=True, resident_bcf=True, **kw)


def _same(tmp_path, path, gt, with_file=True, **kw):
    """--resident-bcf 1 against --on-device 0 on one file: return code, stdout, the -o file and stderr (messages and the error)"""
    rh = U.fetch(path, gt, on_device=False, **kw)
    rd = _resident(path, gt, **kw)
    assert rd[0] == rh[0], (rd[2][-2000:], rh[2][-2000:])
    assert rd[1] == rh[1]
    assert U.plain(rd[2]) == U.plain(rh[2])
    if with_file:
        od = str(tmp_path / "dev.csv")
        fd = _resident(path, gt, out=od, **kw)
        assert fd[0] == rh[0] and fd[1] == "" and open(od, "rb").read() == rh[1].encode() and U.plain(fd[2]) == U.plain(rh[2])
    return rh, rd


def _is_resident(stderr, records=None):
    res = R.rb_line(stderr)
    assert res["resident"] == 1 and res["why"] is None and res["members"] > 0 and res["up"] > 0, res
    assert res["head_bytes"] >= 32 * res["records"]
    assert not U.inflate_lines(stderr)                                 # no part of the file came down whole
    if records is not None:
        assert res["records"] == records
    return res


def _bgzf_file(tmp_path, name, data, block=60000):
    return U.write(tmp_path / name, gm.bgzf(data, block=block))


SHAPES = [(n, r) for n in (1, 63, 64, 65, 257) for r in (1, 7, 300)]


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_generated_files(k, tmp_path):
    n, n_records = SHAPES[k]
    first = 2 ** 31 - n_records if k % 2 else 8
    recs = gm.make_records(n, n_records, seed=3000 + k, first_pos=first, fixed_alleles=True)
    path = _bgzf_file(tmp_path, "in.bcf", gm.bcf_bytes(recs, n), block=(60000, 4096, 9973)[(k // 3 + k) % 3])    # every member size meets every record count
    for j, batch in enumerate((1, 7, 4096)):
        gt = gm.GENOTYPES[(3 * k + j) % 15]
        rh, rd = _same(tmp_path, path, gt, with_file=(j == 2), batch_records=batch)
        assert rh[0] == 0, rh[2][-2000:]
        _is_resident(rd[2], records=n_records)
        records, with_line, redone, up, down = U.fetch_counts(rd[2])
        assert (records, with_line, redone) == (n_records, n_records, 0) and down > 0
        assert up == 32 * with_line                                    # descriptors alone go up: no GL vector is staged


def test_drawn_alleles_put_the_gl_blocks_at_every_residue(tmp_path):
    n = 3
    recs = gm.make_records(n, 60, seed=7000)
    data = gm.bcf_bytes(recs, n)
    gl = R.gl_fields(data, n)
    assert {len(a) for r in recs for a in r["alleles"]} >= {1, 2, 3, 9}
    assert {off & 3 for off, _ in gl} == {0, 1, 2, 3} and any(nv == 15 for _, nv in gl) and len(gl) == 60      # a condition on the input
    raw = U.write(tmp_path / "drawn.raw.bcf", data)
    path = _bgzf_file(tmp_path, "drawn.bcf", data, block=997)
    lines = 0
    for gt in ("AC", "GG", "TA", "A<"):
        want = gm.run_file(raw, gt)
        rh, rd = _same(tmp_path, path, gt, with_file=(gt == "AC"), batch_records=7)
        assert rd[0] == want.returncode == 0 and rd[1] == "".join(want.stdout) and U.plain(rd[2]) == "".join(want.messages)
        _is_resident(rd[2], records=60)
        records, with_line, redone, up, _ = U.fetch_counts(rd[2])
        assert (records, with_line, redone) == (60, want.lines, 0) and up == 32 * with_line
        lines += with_line
    assert lines > 20
    rc, res, se = R.rb_check(path)
    assert rc == 0 and (res["records"], res["flagged"], res["differences"]) == (60, 0, 0) and res["fields"] >= 60, (res, se)


def test_chain_launches(tmp_path):
    """records much shorter than the chain's window (many hops a window), and records about as long as it (each crosses a boundary)"""
    for name, n, n_records in (("short", 1, 300), ("window", 17, 40)):
        recs = gm.make_records(n, n_records, seed=81, fixed_alleles=True, fmt="GL")
        data = gm.bcf_bytes(recs, n)
        walk = R.walk(data, n)
        size = [r["end"] - r["off"] for r in walk]
        if name == "short":
            assert max(size) < 128
        else:                                                          # 17 x 15 floats and a head: the window's 1024 bytes, a little more,
            assert 1024 <= min(size) and max(size) < 1200               # so every record begins inside a window and ends in the next
        path = _bgzf_file(tmp_path, name + ".bcf", data, block=3000)
        for h in (1, 2, 7):
            rc, res, se = R.rb_check(path, h)
            assert rc == 0 and (res["records"], res["flagged"], res["differences"]) == (n_records, 0, 0), (res, se)
            assert res["hops_most"] == h and res["launches"] == n_records // h + 1
        rh, rd = _same(tmp_path, path, "CG", with_file=False, batch_records=64)
        assert rh[0] == 0
        _is_resident(rd[2], records=n_records)


def test_members_of_13_bytes(tmp_path):
    """more members than one inflate call takes: every record and every length word lies across members"""
    recs = gm.make_records(65, 14, seed=77, first_pos=95, fixed_alleles=True)
    data = gm.bcf_bytes(recs, 65)
    path = _bgzf_file(tmp_path, "small_members.bcf", data, block=13)
    rh, rd = _same(tmp_path, path, "CG", with_file=False)
    res = _is_resident(rd[2], records=14)
    assert rh[0] == 0 and res["members"] == -(-len(data) // 13) + 1 > 4096 and U.fetch_counts(rd[2])[:3] == (14, 14, 0)


def _stops(tmp_path, data, gt, at, first_pos, what, raw_name="stop.raw.bcf"):
    want = gm.run_file(U.write(tmp_path / raw_name, data), gt)
    assert want.stop == (what, first_pos + at)
    path = _bgzf_file(tmp_path, "stop.bcf", data, block=7000)
    rh, rd = _same(tmp_path, path, gt, batch_records=7)
    assert rd[0] == 1 and rd[1] == "".join(want.stdout) and rd[1].count("\n") == at
    assert U.plain(rd[2]).startswith("".join(want.messages)) and "position %d" % (first_pos + at) in rd[2]
    _is_resident(rd[2])
    return rd


@pytest.mark.parametrize("place", [0, 3, 6])
def test_a_record_without_gl_stops_the_run_where_the_host_stops(place, tmp_path):
    """batches of 7 records: record 14 + place is the first, a middle or the last of its batch"""
    recs = gm.make_records(65, 30, seed=9, first_pos=100, fixed_alleles=True, fmt="GT:GL")
    at = 14 + place
    recs[at]["keys"] = ["GT"]
    rd = _stops(tmp_path, gm.bcf_bytes(recs, 65), "GT", at, 100, "gl")
    assert "Could not read GL tag at position %d" % (100 + at) in rd[2]


def test_a_genotype_beyond_the_vector_stops_the_run_behind_its_note(tmp_path):
    recs = gm.make_records(65, 30, seed=9, first_pos=100, fixed_alleles=True, fmt="GT:GL")
    at = 17
    for c in recs[at]["cols"]:
        if c["GL"]:
            c["GL"] = ",".join(c["GL"].split(",")[:6])
    rd = _stops(tmp_path, gm.bcf_bytes(recs, 65), "GT", at, 100, "range")          # g = 8
    assert "at most 6 values" in rd[2]


def test_gl_of_type_integer_stops_at_the_first_record(tmp_path):
    recs = gm.make_records(5, 9, seed=10, first_pos=100, fixed_alleles=True)
    rd = _stops(tmp_path, gm.bcf_bytes(recs, 5, gl_type="Integer"), "AC", 0, 100, "gl")
    assert "Could not read GL tag at position 100" in rd[2]


def _goes_on_as_resident_0(tmp_path, path, gt, why, rc=0, **kw):
    rh = U.fetch(path, gt, on_device=False)
    rd = _resident(path, gt, **kw)
    assert rd[0] == rh[0] == rc and rd[1] == rh[1] and U.plain(rd[2]) == U.plain(rh[2]), (rd[2][-1500:], rh[2][-1500:])
    res = R.rb_line(rd[2])
    assert res["resident"] == 0 and why in res["why"], res
    (ln,) = U.inflate_lines(rd[2])                                     # the bytes came through the device inflater all the same
    assert not ln["host"] and ln["members"] > 0 and ln["down"] > 0
    od = str(tmp_path / "dev.csv")
    fd = _resident(path, gt, out=od, **kw)
    assert fd[0] == rc and open(od, "rb").read() == rh[1].encode()
    return res, rd


def test_not_resident_and_says_why(tmp_path):
    n = 5
    recs = gm.make_records(n, 20, seed=21, first_pos=50, fixed_alleles=True)
    data = gm.bcf_bytes(recs, n)
    walk = R.walk(data, n)
    path = _bgzf_file(tmp_path, "small.bcf", data)
    res, rd = _goes_on_as_resident_0(tmp_path, path, "AC", "--resident-max-bytes", resident_max_bytes=1000)
    assert rd[1].count("\n") == 20
    _is_resident(_resident(path, "AC", resident_max_bytes=len(data) + os.path.getsize(path))[2], records=20)      # exactly enough
    # cut inside the last record
    cut = _bgzf_file(tmp_path, "cut.bcf", data[:walk[-1]["off"] + 40])
    res, rd = _goes_on_as_resident_0(tmp_path, cut, "AC", "record 20: a record that ends behind the file", rc=1)
    assert "truncated BCF record" in rd[2] and rd[1] == ""
    # the lengths themselves cut
    cut = _bgzf_file(tmp_path, "cut5.bcf", data[:walk[-1]["off"] + 5])
    _goes_on_as_resident_0(tmp_path, cut, "AC", "record 20: a record's lengths lie outside the file", rc=1)
    # an l_shared of 8 (the record still ends where it ended)
    r = walk[6]
    short = R.patched(R.patched(data, r["off"], "<I", 8), r["off"] + 4, "<I", r["end"] - r["off"] - 16)
    res, rd = _goes_on_as_resident_0(tmp_path, _bgzf_file(tmp_path, "lshared.bcf", short), "AC", "record 7: a shared block shorter than 24 bytes", rc=1)
    # a record whose n_sample differs
    (nfs,) = struct.unpack_from("<I", data, walk[11]["off"] + 28)
    other = R.patched(data, walk[11]["off"] + 28, "<I", (nfs & 0xFF000000) | (n + 1))
    res, rd = _goes_on_as_resident_0(tmp_path, _bgzf_file(tmp_path, "nsample.bcf", other), "AC", "record 12: a sample count other than the header's", rc=1)
    assert "has 6 samples, the header names 5 samples" in rd[2]
    # a shared block longer than a small HEAD_MOST
    longest = max(r["l_shared"] for r in walk)
    rc, chk, se = R.rb_check(path, head_most=longest - 1)
    assert rc == 0 and chk["flagged"] == 1 and "a shared block longer than the head bound" in chk["why"] and chk["head_most"] == longest - 1, (chk, se)
    rc, chk, se = R.rb_check(path, head_most=longest)
    assert rc == 0 and (chk["flagged"], chk["differences"], chk["records"]) == (0, 0, 20), (chk, se)


def test_a_text_file_is_handled_as_under_resident_1(tmp_path):
    recs = gm.make_records(5, 20, seed=21, fixed_alleles=True)
    path = _bgzf_file(tmp_path, "small.vcf.gz", gm.vcf_text(recs, 5).encode())
    rh = U.fetch(path, "AC", on_device=False)
    rd = _resident(path, "AC")
    assert rd[:2] == rh[:2] and rd[0] == 0 and U.plain(rd[2]) == U.plain(rh[2])
    assert U.resident_line(rd[2])["resident"] == 1 and "resident-bcf" not in rd[2]


def test_a_file_the_simulator_wrote(tmp_path):
    """htslib-shaped records: five alleles and fifteen GLs a record, the extended length in every descriptor"""
    out = str(tmp_path / "sim")
    argv = [VCFGL, "-i", os.path.join(DATA, "data3.vcf"), "-o", out, "-O", "b", "--seed", "42", "--depth", "4", "--error-rate", "0.01", "-explode", "1", "-doUnobserved", "4"]

    def simulate():
        r = subprocess.run(argv, capture_output=True, text=True, timeout=U.TIMEOUT)
        return r.returncode, r.stdout, r.stderr
    rc, so, se = U.guarded("vcfgl_hip", simulate)
    assert rc == 0, se[-2000:]
    path = out + ".bcf"
    data = gzip.decompress(open(path, "rb").read())
    names, keys = R.header_of(data)
    gl = R.gl_fields(data, len(names), gl_key=keys["GL"])
    assert gl and any(nv == 15 for _, nv in gl) and len(names) > 1      # a condition on the input: records of fifteen GLs, 0xF5 0x11 0x0F
    lines = 0
    for gt in ("AC", "GG", "T<"):
        rh, rd = _same(tmp_path, path, gt, with_file=(gt == "AC"), batch_records=5)
        assert rh[0] == 0, rh[2][-1500:]
        res = _is_resident(rd[2])
        records, with_line, redone, up, _ = U.fetch_counts(rd[2])
        assert records == res["records"] > 0 and redone == 0 and up == 32 * with_line
        lines += with_line
    assert lines > 0
    rc, chk, se = R.rb_check(path, 7)
    assert rc == 0 and (chk["flagged"], chk["differences"]) == (0, 0) and chk["records"] == res["records"], (chk, se)
