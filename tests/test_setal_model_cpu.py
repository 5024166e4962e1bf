"""The numpy model of misc/setAlleles (tests/setal_model.py) against the tool's own recorded outputs (tests/golden/misc_setalleles):
applied to the parsed data2.vcf and formatted with the writers' number formatter (tests/vcftext_model.py), it gives every record line
of reference/data2_alleles1.vcf and reference/data2_alleles2.vcf byte for byte.  Also the map properties the kernels rely on, and the
TSV reader of the package."""
import os

import numpy as np
import pytest

import setal_model as sm
import vcftext_model as vt
from vcfgl_amd import setalleles

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "misc_setalleles")
NAMES = ["A", "C", "G", "T", "<*>"]


def f32_bits(tok):
    return sm.FLOAT_MISSING if tok == "." else np.float32(float(tok)).view(np.uint32)


def parse(path):
    """the record lines of a VCF as dicts: fixed columns, alleles as codes, DP, QS bits, and per tag a [nG, N] array"""
    recs = []
    for ln in open(path):
        if ln.startswith("#"):
            continue
        c = ln.rstrip("\n").split("\t")
        alleles = [NAMES.index(x) for x in [c[3]] + c[4].split(",")]
        info = dict(kv.split("=") for kv in c[7].split(";"))
        assert c[8] == "DP:GL:PL:GP"
        cols = [s.split(":") for s in c[9:]]
        r = {"fixed": c[:3] + c[5:7], "alleles": alleles, "info_dp": info["DP"], "line": ln,
             "qs": np.array([f32_bits(x) for x in info["QS"].split(",")], np.uint32).view(np.float32),
             "dp": np.array([int(s[0]) for s in cols], np.int32),
             "gl": np.array([[f32_bits(x) for x in s[1].split(",")] for s in cols], np.uint32).T.copy(),
             "pl": np.array([[-2 ** 31 if x == "." else int(x) for x in s[2].split(",")] for s in cols], np.int32).T.copy(),
             "gp": np.array([[f32_bits(x) for x in s[3].split(",")] for s in cols], np.uint32).T.copy()}
        recs.append(r)
    return recs


def render(r, new, out):
    """the record line of the relabelled record"""
    names = [NAMES[a] for a in new]
    qs = ",".join(vt.fmt_float_bits(b) for b in out["qs"].view(np.uint32))
    cols = []
    for s in range(len(r["dp"])):
        cols.append(":".join([str(int(r["dp"][s])), ",".join(vt.fmt_float_bits(b) for b in out["gl"][:, s]),
                              ",".join("." if v == -2 ** 31 else str(int(v)) for v in out["pl"].view(np.int32)[:, s]),
                              ",".join(vt.fmt_float_bits(b) for b in out["gp"][:, s])]))
    f = r["fixed"]
    return "\t".join([f[0], f[1], f[2], names[0], ",".join(names[1:]), f[3], f[4], "DP=%s;QS=%s" % (r["info_dp"], qs), "DP:GL:PL:GP"] + cols) + "\n"


@pytest.fixture(scope="module")
def records():
    return parse(os.path.join(HERE, "data", "data2.vcf"))


@pytest.mark.parametrize("k", [1, 2])
def test_the_model_reproduces_the_tools_recorded_output(records, k):
    targets = setalleles.read_tsv(os.path.join(HERE, "data", "data2_alleles%d.tsv" % k), "<*>")
    want = [ln for ln in open(os.path.join(HERE, "reference", "data2_alleles%d.vcf" % k)) if not ln.startswith("#")]
    assert len(targets) == len(records) == len(want) == 10
    for r, new, line in zip(records, targets, want):
        assert set(new) <= set(r["alleles"])                        # a subset: never the tool's undefined case
        out = sm.relabel_record(r["alleles"], list(new), qs=r["qs"], gl=r["gl"], pl=r["pl"].view(np.uint32), gp=r["gp"])
        assert render(r, new, out) == line


def test_all_twenty_target_lines_are_subsets_and_the_input_has_a_missing_sample(records):
    n = 0
    for k in (1, 2):
        for r, new in zip(records, setalleles.read_tsv(os.path.join(HERE, "data", "data2_alleles%d.tsv" % k))):
            assert set(new) <= set(r["alleles"]) and len(r["alleles"]) == 5
            n += 1
    assert n == 20
    assert any((r["dp"] == 0).any() and (r["gl"] == sm.FLOAT_MISSING).all(axis=0).any() for r in records)


def random_tile(rng, old, N):
    nG = sm.n_gt(len(old))
    gl = (-rng.random((nG, N)) * 30).astype(np.float32)
    gl[rng.integers(0, nG, N), np.arange(N)] = 0.0
    pl = rng.integers(0, 256, (nG, N)).astype(np.int32)
    pl[rng.integers(0, nG, N), np.arange(N)] = 0
    gp = rng.random((nG, N)).astype(np.float32)
    gl, gp = gl.view(np.uint32).copy(), gp.view(np.uint32).copy()
    gl[:, 0] = gp[:, 0] = sm.FLOAT_MISSING                           # a sample without reads
    pl[:, 0] = -2 ** 31
    return rng.random(len(old)).astype(np.float32), gl, pl.view(np.uint32), gp


def test_the_identity_target_leaves_a_normalised_tile_bit_identical():
    rng = np.random.default_rng(3)
    for n in range(2, 6):
        old = [int(c) for c in rng.permutation(5)[:n]]
        qs, gl, pl, gp = random_tile(rng, old, 9)
        # a normalised tile: GL's maximum and PL's minimum are 0; GP in 64ths, so that its float sum is exactly 1
        gp = (rng.multinomial(64, np.ones(sm.n_gt(n)) / sm.n_gt(n), 9).T / 64.0).astype(np.float32).view(np.uint32).copy()
        gp[:, 0] = sm.FLOAT_MISSING
        out = sm.relabel_record(old, old, qs=qs, gl=gl, pl=pl, gp=gp)
        assert np.array_equal(out["gl"], gl) and np.array_equal(out["pl"], pl) and np.array_equal(out["gp"], gp)
        assert np.array_equal(out["qs"].view(np.uint32), qs.view(np.uint32))


def test_two_relabels_equal_the_composed_one_for_subset_targets():
    """the genotype maps compose exactly; so do QS and PL (integers); GL is rounded once per step"""
    rng = np.random.default_rng(4)
    for _ in range(50):
        old = [int(c) for c in rng.permutation(5)]
        mid = [int(c) for c in rng.permutation(old)[:int(rng.integers(3, 6))]]
        new = [int(c) for c in rng.permutation(mid)[:int(rng.integers(2, len(mid) + 1))]]
        g1, g2, g12 = sm.genotype_map(sm.allele_map(old, mid)), sm.genotype_map(sm.allele_map(mid, new)), sm.genotype_map(sm.allele_map(old, new))
        assert [(-1 if h < 0 else g2[h]) for h in g1] == g12
        qs, gl, pl, gp = random_tile(rng, old, 7)
        a = sm.relabel_record(old, mid, qs=qs, pl=pl)
        b = sm.relabel_record(mid, new, qs=a["qs"], pl=a["pl"])
        c = sm.relabel_record(old, new, qs=qs, pl=pl)
        assert np.array_equal(b["pl"], c["pl"]) and np.array_equal(b["qs"].view(np.uint32), c["qs"].view(np.uint32))   # integers: exact
        # GL: scattering commutes exactly; the two subtractions round twice, so the values agree to an ulp of the largest magnitude
        ga = sm.relabel_record(old, mid, gl=gl)["gl"]
        gb = sm.relabel_record(mid, new, gl=ga)["gl"].view(np.float32)
        gc = sm.relabel_record(old, new, gl=gl)["gl"].view(np.float32)
        assert np.array_equal(np.isnan(gb), np.isnan(gc)) and np.allclose(gb[:, 1:], gc[:, 1:], rtol=0, atol=30 * 2.0 ** -22)


def test_the_tsv_reader_and_the_table_builder(tmp_path):
    assert setalleles.parse_line("A\tC,<*>\n") == (0, 1, 4)
    assert setalleles.parse_line("<NON_REF>\tT", "<NON_REF>") == (4, 3)
    for bad in ("A", "A\t", "A\tC\tG", "A\tC,C", "A\tA", "A\tC,G,T,<*>,N", "A\tN", "A\t<NON_REF>", "AC\tG", "A\tC,"):
        with pytest.raises(ValueError):
            setalleles.parse_line(bad)
    t = setalleles.build_table([(0, 1, 4), (3, 2)])
    assert t.dtype == np.int8 and t.tolist() == [[3, 0, 1, 4, -1, -1, 0, 0], [2, 3, 2, -1, -1, -1, 0, 0]]
    for bad in ([(0,)], [(0, 0)], [(0, 5)], [(0, 1, 2, 3, 4, 0)]):
        with pytest.raises(ValueError):
            setalleles.build_table(bad)
    p = tmp_path / "a.tsv"
    p.write_text("A\tC\nG\tT,<*>\n")
    assert setalleles.read_tsv(str(p)) == [(0, 1), (2, 3, 4)]
