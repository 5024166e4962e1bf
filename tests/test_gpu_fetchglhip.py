"""fetchgl_hip on the device (vcfgl_amd/csrc/misc/fetchgl.hip): every byte the device path writes -- the CSV on stdout or in the -o
file, the tool's messages on stderr, the error a run stops with -- is what --on-device 0 writes (which tests/test_fetchglhip_cli_cpu.py
holds against the reference's recorded outputs and against tests/fgl_file_model.py), on the golden inputs and on generated files whose
shapes put workgroup, chunk, 16-byte and batch boundaries everywhere; the share of records handed back to the host; a record whose
value index is out of range at the first, a middle and the last place of a batch; and the tie to vcfgl_hip --fetch-gl.

Every GPU process runs under a timeout; after a process that faulted, aborted or ran out of time nothing more is started."""
import os
import re
import subprocess

import pytest

import fgl_file_model as gm
from vcfgl_amd import fetchgl as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TEST12 = os.path.join(GOLD, "misc_fetchgl", "data", "test12.vcf")
TEST10 = os.path.join(GOLD, "ref_vcf", "reference", "test10", "test10.vcf")
VCFGL = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA3 = os.path.join(GOLD, "ref_vcf", "data", "data3.vcf")
TIMEOUT = 120
_gave_up = []                          # a GPU process faulted, aborted or timed out: nothing more is started


def _check_alive(rc, what):
    if rc in (-6, -11, 134, 139, 124, 137):
        _gave_up.append(what)
        pytest.fail("%s ended with status %d: no further GPU process is started" % (what, rc))


def _device(path, gt, **kw):
    if _gave_up:
        pytest.fail("an earlier GPU process faulted (%s): not started" % _gave_up[0])
    try:
        rc, so, se = F.fetch_file(path, gt, on_device=True, verbose=True, timeout=TIMEOUT, **kw)
    except subprocess.TimeoutExpired:
        _gave_up.append("timeout")
        pytest.fail("fetchgl_hip ran out of time: no further GPU process is started")
    _check_alive(rc, "fetchgl_hip")
    return rc, so, se


def _host(path, gt, **kw):
    return F.fetch_file(path, gt, on_device=False, verbose=True, timeout=TIMEOUT, **kw)


def _counts(stderr):
    m = re.search(r"\[fetchgl\] on-device (\d): records (\d+), with a CSV line (\d+), redone on the host (\d+), bytes sent up (\d+), received (\d+)", stderr)
    assert m, stderr[-2000:]
    return tuple(int(m.group(k)) for k in (2, 3, 4, 5, 6))


def _plain(stderr):
    return "".join(ln for ln in stderr.splitlines(True) if not ln.startswith("[fetchgl]"))


def _same(tmp_path, path, gt, **kw):
    """both paths on one file: return code, stdout, the -o file and stderr (messages and the error) must be equal"""
    oh, od = str(tmp_path / "host.csv"), str(tmp_path / "dev.csv")
    rh, rd = _host(path, gt, **kw), _device(path, gt, **kw)
    assert rd[0] == rh[0], (rd[2][-2000:], rh[2][-2000:])
    assert rd[1] == rh[1]
    assert _plain(rd[2]) == _plain(rh[2])
    fh, fd = _host(path, gt, out=oh, **kw), _device(path, gt, out=od, **kw)
    assert fd[0] == fh[0] == rh[0] and fd[1] == fh[1] == "" and open(od, "rb").read() == open(oh, "rb").read() == rh[1].encode()
    assert _plain(fd[2]) == _plain(rh[2])
    return rh, rd


def test_golden_inputs(tmp_path):
    for path, gts in ((TEST12, ("CC", "AC", "AA", "GT")), (TEST10, ("AC", "CA", "AA", "TT"))):
        lines = 0
        for gt in gts:
            rh, rd = _same(tmp_path, path, gt)
            assert rh[0] == 0, rh[2][-2000:]
            records, with_line, redone, up, down = _counts(rd[2])
            assert redone == 0 and _counts(rh[2])[:3] == (records, with_line, 0)       # the golden files are inside the grammar throughout
            assert (up > 0) == (with_line > 0)
            lines += with_line
        assert lines > 0
    assert _device(TEST12, "CC")[1] == open(os.path.join(GOLD, "misc_fetchgl", "reference", "test12.csv")).read()


SHAPES = [(n, r) for n in (1, 63, 64, 65, 257) for r in (1, 7, 300)]


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_generated_files(k, tmp_path):
    n, n_records = SHAPES[k]
    container = gm.CONTAINERS[k % 4]
    # POS crosses 9 / 10 and 99 / 100 from 8 on, and reaches 2^31 in every other file (a BCF holds no larger one)
    first = 2 ** 31 - n_records + 1 if k % 2 else 8
    recs = gm.make_records(n, n_records, seed=3000 + k, first_pos=first, fixed_alleles=True)
    path = gm.write_file(str(tmp_path / ("in." + container)), recs, n, container)
    for j, batch in enumerate((1, 7, 4096)):
        gt = gm.GENOTYPES[(3 * k + j) % 15]
        rh, rd = _same(tmp_path, path, gt, batch_records=batch)
        assert rh[0] == 0, rh[2][-2000:]
        records, with_line, redone, up, down = _counts(rd[2])
        assert (records, with_line, redone) == (n_records, n_records, 0) and up > 0 and down > 0      # inside the grammar: nothing handed back
    if n_records == 300:                                               # drawn alleles: records without the genotype between those with it
        recs = gm.make_records(n, n_records, seed=4000 + k, first_pos=first)
        path = gm.write_file(str(tmp_path / ("drawn." + container)), recs, n, container)
        rh, rd = _same(tmp_path, path, "AC", batch_records=7)
        records, with_line, redone, _, _ = _counts(rd[2])
        assert rh[0] == 0 and records == 300 and 0 < with_line < 300 and redone == 0


@pytest.mark.parametrize("container", gm.CONTAINERS)
def test_every_value_index(container, tmp_path):
    """the fifteen value indices, dealt over the four containers"""
    recs = gm.make_records(65, 40, seed=77, first_pos=95, fixed_alleles=True)
    path = gm.write_file(str(tmp_path / ("in." + container)), recs, 65, container)
    for g, gt in enumerate(gm.GENOTYPES):
        if g % 4 == gm.CONTAINERS.index(container):
            rh, rd = _same(tmp_path, path, gt, batch_records=16)
            assert rh[0] == 0 and rd[1] == "".join(gm.run_file(path, gt).stdout)


def test_fallback_share(tmp_path):
    recs = gm.make_records(65, 300, seed=5, fixed_alleles=True, odd_share=0.1)
    path = gm.write_file(str(tmp_path / "odd.vcf"), recs, 65, "vcf")
    want = gm.run_file(path, "CG")
    rh, rd = _same(tmp_path, path, "CG", batch_records=64)
    assert rh[0] == 0 and rd[1] == "".join(want.stdout)
    records, with_line, redone, _, _ = _counts(rd[2])
    assert (records, with_line) == (300, 300) and redone == want.redone == _counts(rh[2])[2]
    assert 10 <= redone <= 60                                          # about one record in ten (the generator's share, 300 draws)
    # the same seed without the odd tokens: the device may not pass by handing work back
    recs = gm.make_records(65, 300, seed=5, fixed_alleles=True, odd_share=0.0)
    path = gm.write_file(str(tmp_path / "plain.vcf"), recs, 65, "vcf")
    rh, rd = _same(tmp_path, path, "CG", batch_records=64)
    assert _counts(rd[2])[:3] == (300, 300, 0)


@pytest.mark.parametrize("place", [0, 3, 6])
def test_a_record_out_of_range_stops_the_run_where_the_host_stops(place, tmp_path):
    """batches of 7 records: record 14 + place is the first, a middle or the last of its batch"""
    recs = gm.make_records(65, 30, seed=9, first_pos=100, fixed_alleles=True, fmt="GT:GL")
    at = 14 + place
    for c in recs[at]["cols"]:
        if c["GL"]:
            c["GL"] = ",".join(c["GL"].split(",")[:6])
    path = gm.write_file(str(tmp_path / "range.vcf"), recs, 65, "vcf")
    want = gm.run_file(path, "GT")                                    # g = 8
    assert want.stop == ("range", 100 + at)
    rh, rd = _same(tmp_path, path, "GT", batch_records=7)
    assert rd[0] == 1 and rd[1] == "".join(want.stdout) and rd[1].count("\n") == at
    assert "position %d" % (100 + at) in rd[2] and "at most 6 values" in rd[2] and _plain(rd[2]).startswith("".join(want.messages))
    # a column too few there instead
    recs[at]["cols"].pop()
    gm.write_file(path, recs, 65, "vcf")
    rh, rd = _same(tmp_path, path, "AC", batch_records=7)
    assert rd[0] == 1 and rd[1].count("\n") == at and "64 sample columns" in rd[2]


@pytest.mark.parametrize("gt,extra", [("AC", []), ("A<", ["-doUnobserved", "1"])])
def test_tie_to_the_simulators_fetch_gl(gt, extra, tmp_path):
    """--fetch-gl-value 0 is defined as what the tool reads from the file the run writes: fetchgl_hip on that file gives the run's CSV"""
    for mode, ext in (("v", ".vcf"), ("b", ".bcf")):
        if _gave_up:
            pytest.fail("an earlier GPU process faulted: not started")
        o = str(tmp_path / ("sim_" + mode))
        r = subprocess.run([VCFGL, "-i", DATA3, "-o", o, "-explode", "1", "-d", "3", "-e", "0.05", "--seed", "42", "--fetch-gl", gt, "-O", mode] + extra,
                           capture_output=True, text=True, timeout=300)
        _check_alive(r.returncode, "vcfgl_hip")
        assert r.returncode == 0, r.stderr[-2000:]
        csv = open(o + ".fetchgl.csv").read()
        rh, rd = _same(tmp_path, o + ext, gt)
        assert rd[0] == 0 and rd[1] == csv, rd[2][-2000:]
        assert csv.count("\n") > 0 or gt != "AC"


@pytest.mark.parametrize("n_records", [1023, 1024, 1025, 2049, 4097])
def test_scan_chunk_boundaries(n_records, tmp_path):
    """the offsets scan takes 1024 records a chunk: the default --batch-records gives one batch of up to 4096 records -- 1, 2, 3 and 4
    chunks, the carry from chunk to chunk and both parities of its LDS rows -- and, of 4097 records, a batch of one behind it"""
    for n, container in ((1, "vcf"), (2, "bcf")):
        recs = gm.make_records(n, n_records, seed=5000 + n_records + n, first_pos=8, fixed_alleles=True)
        path = gm.write_file(str(tmp_path / ("in." + container)), recs, n, container)
        rh, rd = _same(tmp_path, path, gm.GENOTYPES[(n_records + n) % 15])
        assert rh[0] == 0, rh[2][-2000:]
        assert _counts(rd[2])[:3] == (n_records, n_records, 0)
