"""The discordance model (tests/disc_model.py) and vcfgl_amd.discordance.format_table against the outputs the reference's
misc/gtDiscordance recorded for its own test files (tests/golden/misc_gtdiscordance), the call rule against the GT of those
files, the host program's refusals, and vgl_disc_table_len.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import disc_model as dm
from vcfgl_amd import _abi
from vcfgl_amd.discordance import format_table, split_table, table_len
from vcfgl_amd.vcfio import read_vcf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "misc_gtdiscordance")
BIN = os.path.join(ROOT, "vcfgl_amd", "bin", "vcfgl_hip")
DATA = os.path.join(ROOT, "tests", "golden", "ref_vcf", "data")


def _vcf(name):
    return read_vcf(os.path.join(GOLD, "data", name))


def _ref(name):
    with open(os.path.join(GOLD, "reference", name)) as fh:
        return fh.read()


def test_mode0_equals_the_reference_output():
    truth = _vcf("truth.vcf")
    table = dm.tally_vcf(truth, _vcf("call.vcf"), use_gq=False)
    assert format_table(table, truth.samples, 0) == _ref("test_doGq0.tsv")


@pytest.mark.parametrize("call", ["call3.vcf", "call3_nogq_withpl.vcf", "call3_nogq_withpl_unobservedAllele.vcf"])
def test_per_sample_gq_table_equals_the_reference_output(call):
    truth = _vcf("truth3.vcf")
    table = dm.tally_vcf(truth, _vcf(call))
    want = _ref("test3_doGq7.tsv")
    assert format_table(table, truth.samples, 6) == want
    assert format_table(table, truth.samples, 7) == want and format_table(table, truth.samples, 8) == want


def test_the_other_layouts_are_sums_of_the_per_sample_table():
    truth = _vcf("truth3.vcf")
    table = dm.tally_vcf(truth, _vcf("call3.vcf"))
    rows6 = [list(map(int, ln.split("\t"))) for ln in format_table(table, truth.samples, 6).splitlines()]
    rows4 = [list(map(int, ln.split("\t"))) for ln in format_table(table, truth.samples, 4).splitlines()]
    rows3 = [list(map(int, ln.split("\t"))) for ln in format_table(table, truth.samples, 3).splitlines()]
    rows5 = [list(map(int, ln.split("\t"))) for ln in format_table(table, truth.samples, 5).splitlines()]
    assert [r[0] for r in rows4] == list(range(1, 130)) == [r[0] for r in rows3]
    for k, r4, r3 in zip(range(1, 130), rows4, rows3):
        per = [r for r in rows6 if r[1] == k]
        assert r4[1:] == [sum(r[2 + j] for r in per) for j in range(8)]
        assert r3[1:] == [r4[1], r4[6]]
    assert rows5 == [[r[0], r[1], r[2], r[7], r[10]] for r in rows6]
    with pytest.raises(ValueError):
        format_table(table, truth.samples, 1)


@pytest.mark.parametrize("call", ["call3_nogq_withpl.vcf", "call3_nogq_withpl_unobservedAllele.vcf"])
def test_ml_call_equals_the_files_gt(call):
    n = 0
    for rec in _vcf(call).records:
        for s in range(len(rec.gts)):
            got = dm.ml_call(rec, s)
            if got is None:
                continue
            assert sorted(got) == sorted(rec.gts[s]), (rec.pos0, s)
            n += 1
    assert n >= 6


def test_model_counts_one_tile_by_hand():
    # one site A,C,<*>: sample 0 calls A/C at GQ 7 (truth A/C: het -> het concordant), sample 1 has no reads, sample 2's best PL sits on
    # a genotype with <*> and is passed over (calls C/C, truth A/A: hom -> hom discordant, GQ = the smallest non-zero PL of ALL genotypes)
    pl = np.full((2, 10, 3), 255, dtype=np.uint8)
    pl[0, :6, 0] = [7, 0, 9, 50, 60, 70]
    pl[0, :6, 2] = [40, 30, 20, 5, 3, 0]
    t = dm.tally([0, -3], [3, 2], [[0, 1, 4, -1, -1], [0, 1, -1, -1, -1]], [[4, 0, 5], [1, 1, 1]], pl, [[0x10, 0x00, 0x00], [0, 0, 0]])
    cell, mis, sites = dm.views(t, 3)
    assert cell[0, dm.HET_HET_CONC, 7] == 1 and cell[2, dm.HOM_HOM_DISC, 3] == 1 and cell.sum() == 2
    assert list(mis) == [0, 1, 0] and list(sites) == [1, 1]


@pytest.mark.parametrize("n", [1, 64, 1000])
def test_table_len(n):
    lib = _abi.load_library()
    assert lib.vgl_disc_table_len(n) == dm.table_len(n) == table_len(n)
    c, m, s = split_table(np.zeros(table_len(n), dtype=np.int64))
    assert c.shape == (n, 6, 128) and m.shape == (n,) and s.shape == (2,)


@pytest.mark.skipif(not os.path.exists(BIN), reason="vcfgl_hip not built")
@pytest.mark.parametrize("flags,names", [
    (["--records", "0"], ["--records", "--gt-discordance"]),
    (["--gt-discordance", "1", "--depth", "inf"], ["--gt-discordance", "--depth inf"]),
    (["--gt-discordance", "1", "--records", "0", "-printPileup", "1"], ["--records", "-printPileup"]),
])
def test_binary_refuses_before_it_touches_a_device(flags, names, tmp_path):
    argv = [BIN, "-i", os.path.join(DATA, "data2.vcf"), "-o", str(tmp_path / "o"), "--seed", "1", "-e", "0.01"]
    if "--depth" not in flags:
        argv += ["--depth", "2"]
    r = subprocess.run(argv + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    for name in names:
        assert name in r.stderr, r.stderr
    assert "HIP device" not in r.stderr and not os.path.exists(str(tmp_path / "o") + ".discordance.tsv")
