"""--device-inflate 1 of fetchgl_hip, setalleles_hip and gtdiscordance_hip (misc/record_file.h: the BGZF members of a record file are
inflated on the GPU by the inflater vcfgl_hip uses): return code, stdout, stderr without the tools' own [...] lines and the output
file's bytes are those of --device-inflate 0, for BGZF text and BGZF BCF, with --on-device 0 and 1; the [input] line shows members
inflated on the device and no fallback.  A file cut into more than 512 members (a second batch) and one of one-byte members.  A file
that is not a clean series of BGZF members, or that holds a damaged member, is read by zlib as with 0, and the line says so.

Every GPU process runs under a timeout; after a process that faulted, aborted or ran out of time nothing more is started."""
import os

import pytest

import fgl_file_model as gm
import gtdisc_model as dm
import miscread_util as U
import sal_file_model as sm

pytestmark = pytest.mark.gpu

N, R = 65, 40


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the generated inputs of the three programs, made once"""
    d = tmp_path_factory.mktemp("miscread")
    f = {}
    recs = gm.make_records(N, R, seed=41, first_pos=95, fixed_alleles=True)
    f["fgl_text"] = gm.vcf_text(recs, N).encode()
    f["fgl_bgz"] = U.write(d / "f.vcf.gz", gm.bgzf(f["fgl_text"]))
    f["fgl_bcf"] = U.write(d / "f.bcf", gm.bgzf(gm.bcf_bytes(recs, N), block=20000))
    srecs = sm.make_records(N, R, seed=42, wide_pl=True)
    f["sal_text"] = sm.vcf_text(srecs, N).encode()
    f["sal_bgz"] = U.write(d / "s.vcf.gz", gm.bgzf(f["sal_text"]))
    f["sal_bcf"] = str(d / "s.bcf")
    sm.write_bcf(f["sal_bcf"], sm.bcf_records(srecs, N, end_every=5), N, "bcf.gz")
    f["sal_tsv"] = U.write(d / "s.tsv", sm.tsv_text(srecs).encode())
    t, c = str(d / "t.vcf"), str(d / "c.vcf")
    dm.write_pair(t, c, N, R, "GT:PL:GQ", seed=43, invariant=False)
    f["gtd_truth_text"], f["gtd_call_text"] = open(t, "rb").read(), open(c, "rb").read()
    f["gtd_truth_bgz"] = U.write(d / "t.vcf.gz", gm.bgzf(f["gtd_truth_text"], block=9000))
    f["gtd_call_bgz"] = U.write(d / "c.vcf.gz", gm.bgzf(f["gtd_call_text"]))
    trecs = []
    for ln in f["gtd_truth_text"].decode().split("\n"):
        if ln and ln[0] != "#":
            col = ln.split("\t")
            trecs.append(dict(pos=int(col[1]), alleles=[col[3]] + ([] if col[4] == "." else col[4].split(",")), keys=["GT"], cols=[{"GT": x} for x in col[9:]]))
    f["gtd_truth_bcf"] = U.write(d / "t.bcf", gm.bgzf(gm.bcf_bytes(trecs, N)))
    crecs = []                                                         # the call file as BCF: its GT alone (-doGQ 0 reads nothing else)
    for ln in f["gtd_call_text"].decode().split("\n"):
        if ln and ln[0] != "#":
            col = ln.split("\t")
            crecs.append(dict(pos=int(col[1]), alleles=[col[3]] + ([] if col[4] == "." else col[4].split(",")), keys=["GT"],
                              cols=[{"GT": x.split(":")[0]} for x in col[9:]]))
    f["gtd_call_bcf"] = U.write(d / "c.bcf", gm.bgzf(gm.bcf_bytes(crecs, N), block=7000))
    return f


def _inflated(stderr, n_files=1):
    """the [input] lines of a run whose files were all inflated on the device"""
    lines = U.inflate_lines(stderr)
    assert len(lines) == n_files, stderr[-2000:]
    for ln in lines:
        assert ln["members"] > 0 and not ln["host"] and ln["why"] is None and ln["up"] > 0 and ln["down"] > 0, ln
    return lines


def _fetch_pair(tmp_path, path, gt, on_device, **kw):
    """fetchgl_hip with the flag at 0 and at 1, to stdout and to a file: everything the two runs write must be equal"""
    o0, o1 = str(tmp_path / "o0.csv"), str(tmp_path / "o1.csv")
    a = U.fetch(path, gt, on_device=on_device, device_inflate=False, **kw)
    b = U.fetch(path, gt, on_device=on_device, device_inflate=True, **kw)
    assert b[0] == a[0] and b[1] == a[1] and U.plain(b[2]) == U.plain(a[2]), (a[2][-1500:], b[2][-1500:])
    assert not U.inflate_lines(a[2])
    fa = U.fetch(path, gt, out=o0, on_device=on_device, device_inflate=False, **kw)
    fb = U.fetch(path, gt, out=o1, on_device=on_device, device_inflate=True, **kw)
    assert fb[0] == fa[0] == a[0] and fb[1] == fa[1] == ""
    if os.path.exists(o0) or os.path.exists(o1):
        assert open(o1, "rb").read() == open(o0, "rb").read() == a[1].encode()
    return a, b


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("kind", ["fgl_bgz", "fgl_bcf"])
def test_fetchgl(kind, on_device, files, tmp_path):
    a, b = _fetch_pair(tmp_path, files[kind], "CG", on_device)
    assert a[0] == 0 and a[1].count("\n") == R, a[2][-1500:]
    _inflated(b[2])
    assert U.fetch_counts(b[2])[:3] == (R, R, 0)


@pytest.mark.parametrize("kind,mode,on_device", [("sal_bgz", "v", False), ("sal_bgz", "z", False), ("sal_bcf", "u", False), ("sal_bcf", "u", True), ("sal_bcf", "b", True)])
def test_setalleles(kind, mode, on_device, files, tmp_path):
    p0, p1 = str(tmp_path / "o0"), str(tmp_path / "o1")
    a = U.set_alleles(files[kind], files["sal_tsv"], p0, mode, on_device=on_device, device_inflate=False)
    b = U.set_alleles(files[kind], files["sal_tsv"], p1, mode, on_device=on_device, device_inflate=True)
    assert a[0] == 0 and b[0] == 0 and b[1] == a[1], (a[2][-1500:], b[2][-1500:])
    assert U.plain(b[2]).replace(p1, "PREFIX") == U.plain(a[2]).replace(p0, "PREFIX")
    ext = {"v": ".vcf", "z": ".vcf.gz", "u": ".bcf", "b": ".bcf"}[mode]
    assert open(p1 + ext, "rb").read() == open(p0 + ext, "rb").read() and os.path.getsize(p0 + ext) > 1000
    _inflated(b[2])
    assert not U.inflate_lines(a[2])


def test_setalleles_text_on_the_device_stays_refused(files, tmp_path):
    rc, so, se = U.set_alleles(files["sal_bgz"], files["sal_tsv"], str(tmp_path / "o"), "v", on_device=True, device_inflate=True)
    assert rc == 1 and "Use --on-device 0" in se and not os.path.exists(str(tmp_path / "o.vcf"))


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("call", ["gtd_call_bgz", "gtd_call_bcf"])
@pytest.mark.parametrize("truth", ["gtd_truth_bgz", "gtd_truth_bcf"])
def test_gtdiscordance(truth, call, on_device, files, tmp_path):
    """both files go through the reader, each as BGZF text and as BGZF BCF (the BCF call file holds GT alone: -doGQ 0)"""
    out = str(tmp_path / "out.tsv")
    for mode in ((0,) if call == "gtd_call_bcf" else (0, 6)):
        a = U.compare(files[truth], files[call], out, do_gq=mode, per_site=True, on_device=on_device, device_inflate=False)
        ta = open(out, "rb").read()
        os.remove(out)
        b = U.compare(files[truth], files[call], out, do_gq=mode, per_site=True, on_device=on_device, device_inflate=True)
        assert a[0] == 0 and b[0] == 0 and b[1] == a[1] and len(a[1]) > 0 and U.plain(b[2]) == U.plain(a[2]), (a[2][-1500:], b[2][-1500:])
        assert open(out, "rb").read() == ta and len(ta) > 0
        lines = _inflated(b[2], 2)                                     # both files go through the reader, the truth file first
        assert [os.path.basename(ln["file"]) for ln in lines] == [os.path.basename(files[truth]), os.path.basename(files[call])]
        assert not U.inflate_lines(a[2])


def test_more_members_than_a_batch_and_members_of_one_byte(files, tmp_path):
    text = files["fgl_text"][:60000]
    text = text[:text.rindex(b"\n") + 1]
    many = U.write(tmp_path / "many.vcf.gz", gm.bgzf(text, block=97))
    a, b = _fetch_pair(tmp_path, many, "AC", True)
    assert a[0] == 0 and a[1].count("\n") > 3
    (ln,) = _inflated(b[2])
    assert ln["members"] == -(-len(text) // 97) + 1 > 512 and ln["down"] == len(text)          # a full batch, a second one, the EOF member
    ones = U.write(tmp_path / "ones.vcf.gz", gm.bgzf(text[:2000], block=1))
    a, b = _fetch_pair(tmp_path, ones, "AC", False)                    # (the text ends inside a line: whatever 0 makes of it, 1 makes too)
    (ln,) = _inflated(b[2])
    assert ln["members"] == 2001 and ln["down"] == 2000


@pytest.mark.parametrize("case", ["plain", "gzip", "crc", "truncated", "trailing"])
def test_a_file_that_is_not_clean_bgzf_is_read_by_zlib(case, files, tmp_path):
    data, why = U.damaged(files["fgl_text"])[case]
    path = U.write(tmp_path / ("in." + case), data)
    for on_device in (False, True):
        a, b = _fetch_pair(tmp_path, path, "CG", on_device)
        assert a[1].count("\n") > 0 or case == "crc"                   # (zlib stops at the damaged member: the first one)
        (ln,) = U.inflate_lines(b[2])
        assert ln["host"] and why in ln["why"] and ln["members"] == 0 and ln["down"] == 0, ln
    # --resident 1: the same bytes, and the line says the file is not resident and why
    host = U.fetch(path, "CG", on_device=False)
    r = U.fetch(path, "CG", on_device=True, device_inflate=True, resident=True)
    assert r[0] == host[0] and r[1] == host[1] and U.plain(r[2]) == U.plain(host[2])
    res = U.resident_line(r[2])
    assert res["resident"] == 0 and why in res["why"] and res["lines"] == 0
    (ln,) = U.inflate_lines(r[2])
    assert ln["host"] and why in ln["why"]
    if case in ("plain", "gzip"):                                       # whatever --resident-max-bytes says, the reason is the file's own
        r = U.fetch(path, "CG", on_device=True, device_inflate=True, resident=True, resident_max_bytes=1000)
        res = U.resident_line(r[2])
        assert r[0] == host[0] and r[1] == host[1] and res["resident"] == 0 and why in res["why"], res
    # the other two programs read through the same reader
    if case in ("plain", "crc"):
        sdata = U.damaged(files["sal_text"])[case][0]
        spath = U.write(tmp_path / ("s." + case), sdata)
        p0, p1 = str(tmp_path / "s0"), str(tmp_path / "s1")
        a = U.set_alleles(spath, files["sal_tsv"], p0, "v", on_device=False, device_inflate=False)
        b = U.set_alleles(spath, files["sal_tsv"], p1, "v", on_device=False, device_inflate=True)
        assert b[0] == a[0] and U.plain(b[2]).replace(p1, "PREFIX") == U.plain(a[2]).replace(p0, "PREFIX")
        assert os.path.exists(p1 + ".vcf") == os.path.exists(p0 + ".vcf") and (not os.path.exists(p0 + ".vcf") or open(p1 + ".vcf", "rb").read() == open(p0 + ".vcf", "rb").read())
        (ln,) = U.inflate_lines(b[2])
        assert ln["host"] and why in ln["why"]
        cpath = U.write(tmp_path / ("c." + case), U.damaged(files["gtd_call_text"])[case][0])
        out = str(tmp_path / "out.tsv")
        a = U.compare(files["gtd_truth_bgz"], cpath, out, do_gq=0, on_device=True, device_inflate=False)
        ta = open(out, "rb").read() if os.path.exists(out) else None
        if ta is not None:
            os.remove(out)
        b = U.compare(files["gtd_truth_bgz"], cpath, out, do_gq=0, on_device=True, device_inflate=True)
        assert b[0] == a[0] and U.plain(b[2]) == U.plain(a[2]) and (open(out, "rb").read() if os.path.exists(out) else None) == ta
        lines = U.inflate_lines(b[2])
        assert len(lines) == 2 and not lines[0]["host"] and lines[1]["host"] and why in lines[1]["why"]
