"""gtdiscordance_hip on the device (vcfgl_amd/csrc/misc/gtdisc.hip): every byte the device path writes -- the tables, the -doGQ 1 / 2
listings, the -perSite lines, the stderr counts and the messages -- is what --on-device 0 writes (which tests/test_gtdisc_cli_cpu.py
holds against the reference's recorded outputs and against tests/gtdisc_model.py), on the golden pairs and on synthetic pairs whose
shapes put batch, workgroup and chunk boundaries everywhere; the share of records handed back to the host, the 16-bit counters of
the tally, and the tie to the tally vcfgl_hip --gt-discordance 1 makes of its own calls.

Every GPU process runs under a timeout; after a process that faulted, aborted or ran out of time nothing more is started."""
import os
import re
import subprocess

import numpy as np
import pytest

import disc_model as dm
import gtdisc_model as gm
from vcfgl_amd import discordance as D
from vcfgl_amd.vcfio import read_vcf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "misc_gtdiscordance", "data")
VCFGL = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(ROOT, "tests", "golden", "ref_vcf", "data")
TIMEOUT = 120
_gave_up = []                          # a GPU process faulted, aborted or timed out: nothing more is started


def _check_alive(rc, what):
    if rc in (-6, -11, 134, 139, 124, 137):
        _gave_up.append(what)
        pytest.fail("%s ended with status %d: no further GPU process is started" % (what, rc))


def _device(truth, call, out, **kw):
    if _gave_up:
        pytest.fail("an earlier GPU process faulted (%s): not started" % _gave_up[0])
    try:
        rc, so, se = D.compare_files(truth, call, out, on_device=True, verbose=True, timeout=TIMEOUT, **kw)
    except subprocess.TimeoutExpired:
        _gave_up.append("timeout")
        pytest.fail("gtdiscordance_hip ran out of time: no further GPU process is started")
    _check_alive(rc, "gtdiscordance_hip")
    return rc, so, se


def _host(truth, call, out, **kw):
    return D.compare_files(truth, call, out, on_device=False, verbose=True, timeout=TIMEOUT, **kw)


def _redone(stderr):
    m = re.search(r"\[gtdisc\] on-device (\d): records (\d+), redone on the host (\d+), text bytes sent up (\d+)", stderr)
    assert m, stderr[-2000:]
    return int(m.group(2)), int(m.group(3)), int(m.group(4))


def _plain(stderr, path):
    """stderr without the --verbose line and with the output file's name taken out"""
    return "".join(ln for ln in stderr.splitlines(True) if not ln.startswith("[gtdisc]")).replace(path, "OUT")


def _same(tmp_path, truth, call, **kw):
    """both paths on one pair: return code, output file, stdout and stderr (messages and counts) must be equal"""
    oh, od = str(tmp_path / "host.tsv"), str(tmp_path / "dev.tsv")
    rh = _host(truth, call, oh, **kw)
    rd = _device(truth, call, od, **kw)
    assert rd[0] == rh[0], (rd[2][-2000:], rh[2][-2000:])
    assert open(od, "rb").read() == open(oh, "rb").read()
    assert rd[1] == rh[1]
    assert _plain(rd[2], od) == _plain(rh[2], oh)
    return rh, rd


@pytest.mark.parametrize("do_gq", range(9))
def test_golden_pairs(do_gq, tmp_path):
    g = lambda n: os.path.join(GOLD, n)
    done = 0
    for truth, call in (("truth.vcf", "call.vcf"), ("truth3.vcf", "call3.vcf"), ("truth3.vcf", "call3_nogq_withpl.vcf"),
                        ("truth3.vcf", "call3_nogq_withpl_unobservedAllele.vcf")):
        for per_site in (False, True) if call == "call3.vcf" else (True,):
            rh, rd = _same(tmp_path, g(truth), g(call), do_gq=do_gq, per_site=per_site)
            done += rh[0] == 0
            if rh[0] == 0:
                assert gm.summary(rd[2]) == gm.summary(rh[2])
                assert _redone(rd[2])[1] == 0                          # the golden files are plain grammar throughout
    assert done >= (4 if do_gq == 0 else 1)


SHAPES = [(n, r) for n in (1, 63, 64, 65, 257) for r in (1, 7, 300)]


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_synthetic_pairs(k, tmp_path):
    n, n_records = SHAPES[k]
    fmt = gm.FORMATS[k % len(gm.FORMATS)]
    truth, call = str(tmp_path / "truth.vcf"), str(tmp_path / "call.vcf")
    # POS crosses 9 / 10 and 99 / 100 from 8 on, and 2^31 in every other file; nSites1 crosses them with 300 records
    gm.write_pair(truth, call, n, n_records, fmt, seed=1000 + k, first_pos=(2 ** 31 - 4 if k % 2 else 8), invariant=True)
    tags = [0, 8] if fmt == "GT:PL" else [7, 8, 0]
    for j, batch in enumerate((1, 7, 4096)):
        mode = tags[(j + k) % len(tags)]
        rh, rd = _same(tmp_path, truth, call, do_gq=mode, per_site=(j != 1), batch_records=batch)
        assert rh[0] == 0, rh[2][-2000:]
        records, redone, up = _redone(rd[2])
        assert records == n_records and redone == 0 and up > 0          # plain grammar: nothing may be handed back
    # the listings need a GQ on every record: the same shapes without invariant records
    if fmt != "GT:PL":
        gm.write_pair(truth, call, n, n_records, fmt, seed=2000 + k, first_pos=(8 if k % 2 else 2 ** 31 - 4), invariant=False)
        for j, batch in enumerate((7, 4096, 1)):
            mode = (1, 2, 6)[(j + k) % 3]
            rh, rd = _same(tmp_path, truth, call, do_gq=mode, per_site=(j == 1), batch_records=batch)
            assert rh[0] == 0, rh[2][-2000:]
            assert _redone(rd[2])[1] == 0
            if mode in (1, 2):
                assert len(open(str(tmp_path / "dev.tsv")).read()) > 0 or n * n_records < 4


def test_generator_reaches_every_cell_and_both_listings(tmp_path):
    truth, call = str(tmp_path / "truth.vcf"), str(tmp_path / "call.vcf")
    gm.write_pair(truth, call, 65, 300, "GT:PL:GQ", seed=77, invariant=False)
    res = gm.compare(truth, call, 2, per_site=True)
    cell, mis, _ = dm.views(res.table, 65)
    assert res.stop is None and (cell.sum(axis=(0, 2)) > 0).all() and mis.sum() > 0
    assert set(np.nonzero(cell.sum(axis=(0, 1)))[0]) >= {1, 9, 10, 99, 100, 127}
    rh, rd = _same(tmp_path, truth, call, do_gq=2, per_site=True, batch_records=64)
    assert open(str(tmp_path / "dev.tsv")).read() == "".join(res.listing) and rd[1] == "".join(res.per_site)
    assert any(len(a) >= 2 for _, al, _, cols in gm.parse(call)[2] for c in cols for a in re.split(r"[/|]", c.split(":")[0]) if a.isdigit() and int(a) >= 10)


@pytest.mark.parametrize("fmt,mode", [("GT:DP:GQ", 2), ("GT:PL", 8)])
def test_fallback_share(fmt, mode, tmp_path):
    truth, call = str(tmp_path / "truth.vcf"), str(tmp_path / "call.vcf")
    gm.write_pair(truth, call, 65, 300, fmt, seed=5, invariant=(mode == 8), odd_share=0.1)
    rh, rd = _same(tmp_path, truth, call, do_gq=mode, per_site=True, batch_records=64)
    assert rh[0] == 0, rh[2][-2000:]
    records, redone, _ = _redone(rd[2])
    assert records == 300 and 0 < redone < 300 and redone == _redone(rh[2])[1]
    assert 10 <= redone <= 60                                          # about one record in ten (the generator's share, 300 draws)
    # the same file without the odd tokens: the device may not pass by handing work back
    gm.write_pair(truth, call, 65, 300, fmt, seed=5, invariant=(mode == 8), odd_share=0.0)
    rh, rd = _same(tmp_path, truth, call, do_gq=mode, per_site=True, batch_records=64)
    assert _redone(rd[2])[:2] == (300, 0)


def test_tally_counters_do_not_wrap(tmp_path):
    """one sample, 70 000 hom-ref records in ONE batch: a bin above 65 535 -- the tally's workgroups take runs of at most 32 768"""
    n_records = 70000
    head = '##fileformat=VCFv4.2\n##contig=<ID=chr1,length=100000>\n##FORMAT=<ID=GT,Number=1,Type=String,Description="g">\n'
    cols = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tind0\n"
    truth, call = str(tmp_path / "truth.vcf"), str(tmp_path / "call.vcf")
    with open(truth, "w") as f:
        f.write(head + cols + "".join("chr1\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t0/0\n" % (p + 1) for p in range(n_records)))
    with open(call, "w") as f:
        f.write(head + '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="q">\n' + cols +
                "".join("chr1\t%d\t.\tA\tC\t.\tPASS\t.\tGT:GQ\t0/0:50\n" % (p + 1) for p in range(n_records)))
    rh, rd = _same(tmp_path, truth, call, do_gq=6, batch_records=100000)
    assert rh[0] == 0 and _redone(rd[2])[:2] == (n_records, 0)
    rows = open(str(tmp_path / "dev.tsv")).read().split("\n")
    assert rows[49] == "0\t50\t0\t0\t0\t0\t0\t70000\t70000\t0\t70000"


@pytest.mark.skipif(not os.path.exists(VCFGL), reason="vcfgl_hip not built")
def test_tie_to_the_tally_of_the_simulator(tmp_path):
    """vcfgl_hip tallies its own maximum-likelihood calls; the same calls written as a call file (GT:PL, no GQ) and compared with
    the truth file under -doGQ 8 give that run's table"""
    if _gave_up:
        pytest.fail("an earlier GPU process faulted: not started")
    o = str(tmp_path / "sim")
    r = subprocess.run([VCFGL, "-i", os.path.join(DATA, "data3.vcf"), "-o", o, "--seed", "42", "-e", "0.05", "-O", "v", "-printTruth", "1", "-addPL", "1",
                        "--gt-discordance", "1", "--discordance-gq", "6", "-explode", "1", "-d", "3"], capture_output=True, text=True, timeout=300)
    _check_alive(r.returncode, "vcfgl_hip")
    assert r.returncode == 0, r.stderr[-2000:]
    truth, recs = read_vcf(o + ".truth.vcf"), read_vcf(o + ".vcf")
    n = len(truth.samples)
    head = [h for h in recs.header_lines if not h.startswith("##FORMAT=<ID=GQ,")]
    lines, left_out = [], 0
    for rec in recs.records:
        calls = [dm.ml_call(rec, s) if rec.samples[s]["DP"][0] not in (".", "0") else None for s in range(n)]
        if any(c is not None and (rec.alleles[c[0]].startswith("<") or rec.alleles[c[1]].startswith("<")) for c in calls):
            left_out += 1                                              # (the tally never calls the unobserved allele: expected 0)
            continue
        nG = len(rec.alleles) * (len(rec.alleles) + 1) // 2
        cols = []
        for s in range(n):
            pl = rec.samples[s]["PL"]
            cols.append("./.:" + ",".join(["."] * nG) if calls[s] is None else "%d/%d:%s" % (calls[s][0], calls[s][1], ",".join(pl)))
        lines.append("\t".join([rec.chrom, str(rec.pos0 + 1), ".", rec.alleles[0], ",".join(rec.alleles[1:]) or ".", ".", "PASS", ".", "GT:PL"] + cols))
    assert left_out == 0 and left_out < 0.1 * len(recs.records) and len(lines) > 0
    call = str(tmp_path / "call.vcf")
    with open(call, "w") as f:
        f.write("\n".join(head + ["#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(truth.samples)] + lines) + "\n")
    rh, rd = _same(tmp_path, o + ".truth.vcf", call, do_gq=8)
    assert rd[0] == 0, rd[2][-2000:]
    assert open(str(tmp_path / "dev.tsv")).read() == open(o + ".discordance.tsv").read()


@pytest.mark.parametrize("n_records", [1023, 1024, 1025, 2049, 4097])
def test_scan_chunk_boundaries(n_records, tmp_path):
    """the offsets scan takes 1024 records a chunk: the default --batch-records gives one batch of up to 4096 records -- 1, 2, 3 and 4
    chunks, the carry from chunk to chunk and both parities of its LDS rows -- and, of 4097 records, a batch of one behind it.
    -doGQ 2 with -perSite 1: both rows of the scan carry lengths; -doGQ 0 with -perSite 1: the listing's row is all zeros"""
    truth, call = str(tmp_path / "truth.vcf"), str(tmp_path / "call.vcf")
    for n, mode in ((1, 2), (2, 0)):
        gm.write_pair(truth, call, n, n_records, "GT:GQ", seed=3000 + n_records + n, invariant=False)
        rh, rd = _same(tmp_path, truth, call, do_gq=mode, per_site=True)
        assert rh[0] == 0, rh[2][-2000:]
        assert _redone(rd[2])[:2] == (n_records, 0)
        assert len(rd[1]) > 0 and len(open(str(tmp_path / "dev.tsv")).read()) > 0      # -perSite lines; the listing or the table
